// sn_inflate.hpp — inflation of occupancy grids by the robot's radius (sn_inflate_grid; the contract is in
// include/stereonet_hip.h, the numpy twin is hobot_stereonet_amd/inflate.py).  Everything on the device is integer: the one
// piece of floating point, the cost table T[d2], is built on the host (in_table) and uploaded.
//
//   k_inflate     grid (tiles of a map, maps), 256 or 1024 threads.  A workgroup owns a 64 x 16 tile of one map and reads the
//                 tile with a halo of R cells on every side (at R = 64: 192 x 144 cells).  The obstacles of that window are kept
//                 as BIT ROWS in LDS: row r of the window is three 64-bit words (the 64 columns left of the tile, the tile's,
//                 the 64 right of it; columns further than R from the tile and cells outside the grid are 0), each word one
//                 __ballot of a wave that loaded 64 consecutive bytes of occ.  At most 144 x 3 x 8 = 3456 bytes, and no global
//                 scratch.
//                 A lane owns a column and a wave four rows of the tile (four waves) or one (sixteen): the walk is a chain of
//                 dependent LDS reads, so a call whose workgroups are all resident at once is bound by one workgroup's latency
//                 and takes the wide form, in which the rows run side by side; a larger call is bound by throughput and takes
//                 the narrow one, whose workgroups pack the CUs better (in_waves; SN_INFLATE_WAVES forces either).
//                 For its pixel a lane walks dy = 0, 1, 2, ...: rows
//                 y - dy and y + dy are ORed (wave-uniform LDS reads: a broadcast), the nearest set bit left and right of the
//                 lane's column comes from two shifts and a count of trailing / leading zeros, and best = min(hx^2 + dy^2).  The
//                 walk stops at dy^2 >= best; best starts at R^2 + 1 ("not reached"), so |dy| <= R needs no test of its own and
//                 the result is the exact minimum wherever that is <= R^2.
//                 A window without an obstacle - most of a real map - skips the walk and the table: every cell is 0 or 255.
//                 T (at most 4097 bytes) is staged in LDS by the workgroups that walk.
//                 Outputs are byte-wide (uint16 for dist2) at any address and any gw: a wave stores 64 consecutive elements.
//                 stats: the five classes are counted per wave by __ballot / popcount, added to an LDS table by one lane per
//                 wave, and after a barrier one global atomicAdd per workgroup and non-zero counter (integer, order-free).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/stereonet_hip.h"

namespace sn {

constexpr int kInMaxR = SN_INFLATE_MAX_R;
constexpr int kInMaxCells = 4096;       // gw, gh
constexpr int kInTileW = 64, kInTileH = 16;
constexpr int kInMaxRows = kInTileH + 2 * kInMaxR;
constexpr int kInLoads = 8;             // bytes of occ a lane has in flight while the bit rows are built

// nullptr, or why sn_inflate_table refuses the parameters; *R_out = R of the contract
inline const char* in_params_check(const sn_inflate_params* p, int* R_out) {
  if (!p) return "a NULL pointer";
  if (!std::isfinite(p->cell_m) || !(p->cell_m > 0.f)) return "cell_m must be finite and positive";
  if (!std::isfinite(p->inscribed_radius_m) || p->inscribed_radius_m < 0.f) return "inscribed_radius_m must be finite and not negative";
  if (!std::isfinite(p->inflation_radius_m) || p->inflation_radius_m < p->inscribed_radius_m)
    return "inflation_radius_m must be finite and at least inscribed_radius_m";
  if (!std::isfinite(p->cost_scaling) || p->cost_scaling < 0.f) return "cost_scaling must be finite and not negative";
  const double r = ceil((double)p->inflation_radius_m / (double)p->cell_m);
  if (!(r <= (double)kInMaxR)) return "the inflation radius must be at most 64 cells";
  if (p->lethal_min < 1 || p->lethal_min > 100) return "lethal_min must be 1..100";
  if (p->flags & ~SN_INFLATE_UNKNOWN) return "flags has bits other than SN_INFLATE_UNKNOWN";
  *R_out = (int)r;
  return nullptr;
}

// T of the contract for parameters in_params_check accepts: R*R + 1 bytes.  false: the table increases somewhere.
inline bool in_table(const sn_inflate_params* p, int R, uint8_t* T) {
  const double cell = (double)p->cell_m, inscribed = (double)p->inscribed_radius_m, inflation = (double)p->inflation_radius_m,
               scaling = (double)p->cost_scaling;
  T[0] = 254;
  for (int d2 = 1; d2 <= R * R; ++d2) {
    const double dist = sqrt((double)d2) * cell;
    if (dist <= inscribed) T[d2] = 253;
    else if (dist > inflation) T[d2] = 0;
    else T[d2] = (uint8_t)(252.0 * exp(-scaling * (dist - inscribed)));
    if (T[d2] > T[d2 - 1]) return false;
  }
  return true;
}

// waves per workgroup of a call of `workgroups` tiles on `num_cu` CUs; forced: SN_INFLATE_WAVES (4 or 16; anything else: by size).
// Two 1024-thread workgroups fit a CU, so up to 2 * num_cu of them start at once and the call takes one workgroup's time.
inline int in_waves(long long workgroups, int num_cu, int forced) {
  if (forced == 4 || forced == 16) return forced;
  return workgroups <= 2ll * num_cu ? 16 : 4;
}

struct InArgs {
  const int8_t* occ;       // [maps][gh][gw]
  const uint8_t* table;    // [R*R + 1]
  uint8_t* cost;           // nullable
  int8_t* grid;            // nullable
  uint16_t* dist2;         // nullable
  uint32_t* stats;         // nullable: [maps][5], zeroed before the launch
  int gw, gh, tiles_x, R, lethal_min, flags;
};

// the distance from column lx of the middle word to the nearest set bit of the 192-bit row (w0, w1, w2); 4096 without one
__device__ __forceinline__ int in_nearest(unsigned long long w0, unsigned long long w1, unsigned long long w2, int lx) {
  const unsigned long long right = w1 >> lx, left = w1 << (63 - lx);      // bit lx of w1 at bit 0, and at bit 63
  const int r = right ? __builtin_ctzll(right) : (w2 ? 64 - lx + __builtin_ctzll(w2) : 4096);
  const int l = left ? __builtin_clzll(left) : (w0 ? lx + 1 + __builtin_clzll(w0) : 4096);
  return min(r, l);
}

// grid (tiles_x * tiles_y, maps), 64 * WAVES threads: a wave owns kInTileH / WAVES rows of the tile
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_inflate(InArgs a) {
  __shared__ unsigned long long bits[kInMaxRows][3];
  __shared__ __align__(16) uint8_t T[kInMaxR * kInMaxR + 16];
  __shared__ uint32_t cnt[5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int x0 = tx * kInTileW, y0 = ty * kInTileH, R = a.R, R2 = R * R;
  const size_t cells = (size_t)a.gw * a.gh;
  const int8_t* occ = a.occ + (size_t)blockIdx.y * cells;
  if (threadIdx.x < 5) cnt[threadIdx.x] = 0;
  // the bit rows of the window: item = (row, word), dealt to the waves
  const int rows = kInTileH + 2 * R;
  bool any = false;
  for (int base = wave; base < rows * 3; base += WAVES * kInLoads) {      // kInLoads loads in flight, then their ballots
    int v[kInLoads];
#pragma unroll
    for (int u = 0; u < kInLoads; ++u) {
      const int item = base + WAVES * u, r = item / 3, j = item - r * 3;
      const int y = y0 - R + r, x = x0 + (j - 1) * 64 + lane;
      const bool in = item < rows * 3 && y >= 0 && y < a.gh && x >= 0 && x < a.gw && x >= x0 - R && x < x0 + kInTileW + R;
      // every lane loads, from an address clamped into the map, so that no branch separates the loads
      const int o = occ[(size_t)min(max(y, 0), a.gh - 1) * a.gw + min(max(x, 0), a.gw - 1)];
      v[u] = in ? o : -128;
    }
#pragma unroll
    for (int u = 0; u < kInLoads; ++u) {
      const int item = base + WAVES * u, r = item / 3, j = item - r * 3;
      if (item < rows * 3) {      // wave-uniform
        const unsigned long long w = __ballot(v[u] >= a.lethal_min);
        any = any || w != 0;
        if (lane == 0) bits[r][j] = w;
      }
    }
  }
  const bool walk = __syncthreads_or(any) != 0;      // also: cnt and bits are written
  if (walk) {
    for (int i = threadIdx.x; i <= R2; i += 64 * WAVES) T[i] = a.table[i];
    __syncthreads();
  }
  const int x = x0 + lane;
  uint32_t n254 = 0, n253 = 0, nmid = 0, n0 = 0, n255 = 0;      // of the wave, in every lane
#pragma unroll 1
  for (int k = 0; k < kInTileH / WAVES; ++k) {
    const int ly = wave * (kInTileH / WAVES) + k, y = y0 + ly;
    const bool live = x < a.gw && y < a.gh;
    int best = R2 + 1;
    if (walk && live) {
      const int rc = ly + R;
      const int h0 = in_nearest(bits[rc][0], bits[rc][1], bits[rc][2], lane);
      best = min(best, h0 * h0);      // h0 <= 4096
      for (int dy = 1; dy * dy < best; ++dy) {      // dy <= R: best <= R2 + 1
        const unsigned long long* up = bits[rc - dy];
        const unsigned long long* dn = bits[rc + dy];
        const int hx = in_nearest(up[0] | dn[0], up[1] | dn[1], up[2] | dn[2], lane);
        best = min(best, hx * hx + dy * dy);
      }
    }
    const size_t at = (size_t)blockIdx.y * cells + (size_t)y * a.gw + x;
    int c = 0, cost = 0;
    if (live) {
      const int o = occ[(size_t)y * a.gw + x];
      if (best <= R2) c = walk ? T[best] : 0;
      const bool take = o >= 0 || ((a.flags & SN_INFLATE_UNKNOWN) ? c > 0 : c >= 253);
      cost = take ? c : 255;
      if (a.cost) a.cost[at] = (uint8_t)cost;
      if (a.grid) a.grid[at] = (int8_t)(cost == 0 ? 0 : cost == 255 ? -1 : cost == 254 ? 100 : cost == 253 ? 99 : 1 + 97 * (cost - 1) / 251);
      if (a.dist2) a.dist2[at] = (uint16_t)(best <= R2 ? best : 0xFFFF);
    }
    if (a.stats) {      // wave-uniform
      n254 += __popcll(__ballot(live && cost == 254));
      n253 += __popcll(__ballot(live && cost == 253));
      nmid += __popcll(__ballot(live && cost >= 1 && cost <= 252));
      n0 += __popcll(__ballot(live && cost == 0));
      n255 += __popcll(__ballot(live && cost == 255));
    }
  }
  if (a.stats) {
    if (lane == 0) {
      if (n254) atomicAdd(cnt + 0, n254);
      if (n253) atomicAdd(cnt + 1, n253);
      if (nmid) atomicAdd(cnt + 2, nmid);
      if (n0) atomicAdd(cnt + 3, n0);
      if (n255) atomicAdd(cnt + 4, n255);
    }
    __syncthreads();
    if (threadIdx.x < 5 && cnt[threadIdx.x]) atomicAdd(a.stats + (size_t)blockIdx.y * 5 + threadIdx.x, cnt[threadIdx.x]);
  }
}

}  // namespace sn
