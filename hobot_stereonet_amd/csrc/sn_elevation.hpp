// sn_elevation.hpp — rolling elevation map and step-height traversability, two int16 planes per stream (sn_elevation_push; the
// contract is in include/stereonet_hip.h, the numpy twin is hobot_stereonet_amd/elevation.py).  Below the pose quantisation
// everything is integer or a single rounded fp32 operation, and every accumulator is an integer, so the bytes do not depend
// on the order of arrival.
//
//   k_el_clear    one launch starts the accumulators of all n frames (cnt = 0, fmax = INT32_MIN, fmin = INT32_MAX) and stats.
//   k_el_scatter  grid (column blocks * row chunks, maps of the slice), 256 lanes = 256 output columns, the obstacle stage's
//                 walk: a lane owns one column and goes down the rows of its chunk, so consecutive lanes read consecutive
//                 words.  The accumulators of a frame depend on its map, its mount and its pose alone, not on the state, so
//                 every frame of a call is scattered in one launch.  A column of pixels mostly stays in one cell: the lane
//                 keeps its current cell (count, maximum, minimum) in registers, and the lanes of a wave that leave their
//                 cells at the same row flush together (el_wave_flush: the runs of equal cells are folded with shuffles, the
//                 first lane of a run sends the three atomics).  Atomics per run, not per point.
//   k_el_fuse     grid (slot chunks, streams present in the slice), 256 threads: k_costmap's shape.  A lane owns ONE slot of one
//                 stream's torus and walks that stream's frames with hi and lo in registers: the state is read once before the
//                 first frame (not at all for a fresh stream) and written once after the last.  Per frame 12 bytes of
//                 accumulators are read and the unrolled hi and lo (4 bytes) written, into the caller's planes or the scratch.
//                 stats {known, fused, points}: wave sums by shuffles, an LDS table [frame][3], one global atomic per
//                 workgroup, frame and non-zero counter.
//   k_el_verdict  grid (tiles, n), 256 threads, a tile of 64 x 16 cells with a halo of `radius` in LDS.  The rise of a cell is
//                 max(max hi over N - lo_c, hi_c - min lo over N), so the neighbourhood is a separable maximum of hi and minimum
//                 of lo: rows first (into a second LDS table), then columns.  Unknown and outside cells hold the identities
//                 (hi = -32768, lo = 32767).  stats {lethal}: one atomic per workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sn_obstacles.hpp"      // ob_row, ob_height_mm, ob_range, kObAhead
#include "sn_streams.hpp"        // the group lists and the torus

namespace sn {

constexpr int kElMaxWindow = 4096;      // mw, mh
constexpr int kElUnknown = -32768;
constexpr int kElTileW = 64, kElTileH = 16, kElMaxRadius = 3;

struct ElClearArgs {
  uint32_t* cnt;
  int32_t* fmax;
  int32_t* fmin;
  uint32_t* stats;      // nullable
  size_t cells, n_stats;      // n * mh * mw, n * 4
};

struct ElScatterArgs {
  PcArgs pc;              // raw (of the slice), W, H, Wo, Ho, step, scale, fB, fx, fy, cx, cy, zmin, zmax
  uint32_t* cnt;          // [m][mh*mw] of the slice, unrolled
  int32_t* fmax;
  int32_t* fmin;
  float m[12];
  const float* mounts;    // MOUNTS: map k's mount is the twelve floats at mounts + k * mount_stride, and m is not used
  int mount_stride;
  float k256f, range_max;
  int zmin_mm, zmax_mm;
  int mw, mh;
  int chunks, rows;       // row chunks per column block, output rows per chunk
  int q[kSlice][6];     // per map of the slice: tx, ty, cq, sq, ox, oy
};

struct ElFuseArgs {
  const uint32_t* cnt;    // [m][mh*mw] of the slice
  const int32_t* fmax;
  const int32_t* fmin;
  int16_t* hi;            // [m][mh][mw] of the slice, unrolled: the caller's or the scratch, never null
  int16_t* lo;
  uint32_t* stats;        // nullable: [m][4], zeroed before the launch
  int16_t* S;             // state: hi [streams][mh][mw], then lo at lo_off
  size_t lo_off;
  int mw, mh, min_points, alpha;
  StreamGroups g;         // the slice's maps, sorted by stream; fresh: all unknown, no previous origin
  TorusPrev t;
  int org[kSlice][2];     // per map of the slice: ox, oy
};

struct ElVerdictArgs {
  const int16_t* hi;      // [n][mh][mw]
  const int16_t* lo;
  int8_t* trav;           // nullable
  uint16_t* rise;         // nullable
  uint32_t* stats;        // nullable: [n][4]
  int mw, mh, radius, max_step, tiles_x;
};

__global__ __launch_bounds__(256) void k_el_clear(ElClearArgs a) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < a.cells; i += (size_t)gridDim.x * 256) {
    a.cnt[i] = 0u;
    a.fmax[i] = INT32_MIN;
    a.fmin[i] = INT32_MAX;
    if (i < a.n_stats) a.stats[i] = 0u;      // n * 4 <= n * mh * mw only from 4 cells on: the tail below covers the rest
  }
  if (blockIdx.x == 0)
    for (size_t i = a.cells + threadIdx.x; i < a.n_stats; i += 256) a.stats[i] = 0u;
}

// the unrolled index (cy - oy) * mw + (cx - ox) of the window cell a base-frame point falls in, or -1
__device__ __forceinline__ int el_cell(const ElScatterArgs& a, const int* q, float xb, float yb) {
#pragma clang fp contract(off)
  const float sxf = floorf(xb * a.k256f), syf = floorf(yb * a.k256f);
  const float lim = 1073741824.f;
  if (!(fabsf(sxf) < lim && fabsf(syf) < lim)) return -1;
  const long long sx = (long long)sxf, sy = (long long)syf, cq = q[2], sq = q[3];
  const long long wx = (long long)q[0] + ((cq * sx - sq * sy + (1ll << 29)) >> 30);
  const long long wy = (long long)q[1] + ((sq * sx + cq * sy + (1ll << 29)) >> 30);
  const long long cx = (wx >> 8) - q[4], cy = (wy >> 8) - q[5];
  if (cx < 0 || cx >= a.mw || cy < 0 || cy >= a.mh) return -1;
  return (int)cy * a.mw + (int)cx;
}

// A flush by the whole wave, as ob_wave_flush: every run of lanes with one cell is folded with shuffles and its first lane sends
// the atomics.  cur < 0: the lane has nothing to send.
__device__ __forceinline__ void el_wave_flush(int cur, uint32_t n_pt, int zmax, int zmin, uint32_t* cnt, int32_t* fmax, int32_t* fmin) {
  const int lane = threadIdx.x & 63;
  const int before = __shfl_up(cur, 1);
  const bool head = lane == 0 || before != cur;
  const int run = __popcll(__ballot(head) & (~0ull >> (63 - lane)));      // the runs are numbered, so equal numbers are contiguous
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int run_o = __shfl_down(run, o), hi_o = __shfl_down(zmax, o), lo_o = __shfl_down(zmin, o);
    const uint32_t n_o = __shfl_down(n_pt, o);
    if (lane + o < 64 && run_o == run) n_pt += n_o, zmax = max(zmax, hi_o), zmin = min(zmin, lo_o);
  }
  if (!head || cur < 0 || !n_pt) return;
  atomicAdd(cnt + cur, n_pt);
  atomicMax(fmax + cur, zmax);
  atomicMin(fmin + cur, zmin);
}

// grid (column blocks * chunks, maps of the slice), 256 lanes = 256 output columns
template <bool MOUNTS>
__global__ __launch_bounds__(256) void k_el_scatter(ElScatterArgs a) {
  const int k = blockIdx.y;
  float own[12];      // MOUNTS: the map's mount, the same for every lane
  if (MOUNTS) {
#pragma unroll
    for (int e = 0; e < 12; ++e) own[e] = a.mounts[(size_t)k * a.mount_stride + e];
  }
  const float* m = MOUNTS ? own : a.m;
  const int* q = a.q[k];
  const int cblock = blockIdx.x / a.chunks, chunk = blockIdx.x - cblock * a.chunks;
  const int j = cblock * 256 + threadIdx.x, u = j * a.pc.step;
  const int i0 = chunk * a.rows, i1 = min(i0 + a.rows, a.pc.Ho);
  const size_t cells = (size_t)a.mw * a.mh;
  uint32_t* cnt = a.cnt + (size_t)k * cells;
  int32_t* fmax = a.fmax + (size_t)k * cells;
  int32_t* fmin = a.fmin + (size_t)k * cells;

  // the lane's run: the cell it is in, with what it has seen of it
  int cur = -1, zmax = INT32_MIN, zmin = INT32_MAX;
  uint32_t n_pt = 0;
  // Every lane of the wave walks the same rows (a column beyond Wo reads nothing), so the wave meets at one point per row
  const bool live = j < a.pc.Wo;
  const int32_t* col = a.pc.raw + (size_t)k * a.pc.H * a.pc.W + (live ? u : 0);
  const size_t pitch = (size_t)a.pc.step * a.pc.W;
  for (int ib = i0; ib < i1; ib += kObAhead) {
    int32_t r[kObAhead];
#pragma unroll
    for (int e = 0; e < kObAhead; ++e) r[e] = live && ib + e < i1 ? col[(size_t)(ib + e) * pitch] : 0;
#pragma unroll
    for (int e = 0; e < kObAhead; ++e) {
      if (ib + e >= i1) break;      // the same for the whole workgroup
      const float z = pc_depth(r[e], a.pc.scale, a.pc.fB);
      int c = -1, zmm = 0;
      if (pc_valid(r[e], z, a.pc)) {
        const float4 p = pc_point<false>(a.pc, nullptr, u, (ib + e) * a.pc.step, z);
        const float zb = ob_row(m + 8, p.x, p.y, p.z);
        if (zb == zb) {
          zmm = ob_height_mm(zb);
          if (a.zmin_mm <= zmm && zmm <= a.zmax_mm) {
            const float xb = ob_row(m, p.x, p.y, p.z), yb = ob_row(m + 4, p.x, p.y, p.z);
            if (ob_range(xb, yb) <= a.range_max) c = el_cell(a, q, xb, yb);
          }
        }
      }
      const bool leaves = c >= 0 && cur >= 0 && c != cur;
      if (__any(leaves)) {
        el_wave_flush(leaves ? cur : -1, n_pt, zmax, zmin, cnt, fmax, fmin);
        if (leaves) cur = -1;
      }
      if (c >= 0) {
        if (c != cur) cur = c, n_pt = 0, zmax = INT32_MIN, zmin = INT32_MAX;
        ++n_pt;
        zmax = max(zmax, zmm), zmin = min(zmin, zmm);
      }
    }
  }
  el_wave_flush(cur, n_pt, zmax, zmin, cnt, fmax, fmin);      // every lane of the wave, its columns beyond Wo included
}

__device__ __forceinline__ int el_clamp(int v) { return min(max(v, -32767), 32767); }

// grid (ceil(mh*mw / 256), groups)
__global__ __launch_bounds__(256) void k_el_fuse(ElFuseArgs a) {
  __shared__ uint32_t tab[kSlice][3];
  const int g = blockIdx.y, f0 = a.g.first[g], f1 = a.g.first[g + 1];
  const int cells = a.mw * a.mh;      // <= 2^24
  const int p = blockIdx.x * 256 + threadIdx.x;
  const bool live = p < cells;
  const int j = live ? p / a.mw : 0, i = live ? p - j * a.mw : 0;
  if (a.stats && (int)threadIdx.x < (f1 - f0) * 3) tab[threadIdx.x / 3][threadIdx.x % 3] = 0;
  __syncthreads();
  const size_t sp = (size_t)a.g.stream[g] * cells + p;
  bool seen = !a.g.fresh[g];
  int pox = a.t.pox[g], poy = a.t.poy[g];
  int hi = kElUnknown, lo = kElUnknown;
  if (live && seen) hi = a.S[sp], lo = a.S[a.lo_off + sp];
#pragma unroll 1
  for (int f = f0; f < f1; ++f) {
    const int k = a.g.map[f], ox = a.org[k][0], oy = a.org[k][1];
    uint32_t n_known = 0, n_fused = 0, n_pts = 0;
    if (live) {
      const int ui = torus_unroll(i, torus_mod(ox, a.mw), a.mw), uj = torus_unroll(j, torus_mod(oy, a.mh), a.mh);
      torus_if_rolled(seen, i, j, ox + ui, oy + uj, pox, poy, a.mw, a.mh, [&] { hi = lo = kElUnknown; });
      const size_t u = (size_t)k * cells + (size_t)uj * a.mw + ui;
      n_pts = a.cnt[u];
      if (n_pts >= (uint32_t)a.min_points) {
        const int fx = a.fmax[u], fn = a.fmin[u];
        if (hi == kElUnknown) {
          hi = el_clamp(fx), lo = el_clamp(fn);
        } else {
          hi = el_clamp(hi + (((fx - hi) * a.alpha + 128) >> 8));
          lo = el_clamp(lo + (((fn - lo) * a.alpha + 128) >> 8));
        }
        n_fused = 1;
      }
      n_known = hi != kElUnknown;
      a.hi[u] = (int16_t)hi;
      a.lo[u] = (int16_t)lo;
    }
    seen = true, pox = ox, poy = oy;
    if (a.stats) {      // wave-uniform
      uint32_t kf = n_known | (n_fused << 16);      // a wave's sums are at most 64
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {
        kf += __shfl_xor(kf, s);
        n_pts += __shfl_xor(n_pts, s);
      }
      if ((threadIdx.x & 63) == 0) {
        uint32_t* c = tab[f - f0];
        if (kf & 0xffffu) atomicAdd(c + 0, kf & 0xffffu);
        if (kf >> 16) atomicAdd(c + 1, kf >> 16);
        if (n_pts) atomicAdd(c + 2, n_pts);
      }
    }
  }
  if (live && f1 > f0) a.S[sp] = (int16_t)hi, a.S[a.lo_off + sp] = (int16_t)lo;
  if (a.stats) {
    __syncthreads();
    if ((int)threadIdx.x < (f1 - f0) * 3) {
      const int f = threadIdx.x / 3, w = threadIdx.x % 3;
      const uint32_t v = tab[f][w];
      if (v) atomicAdd(a.stats + (size_t)a.g.map[f0 + f] * 4 + (w == 0 ? 0 : w + 1), v);      // {known, -, fused, points}
    }
  }
}

// grid (tiles_x * tiles_y, n)
__global__ __launch_bounds__(256) void k_el_verdict(ElVerdictArgs a) {
  constexpr int HW = kElTileW + 2 * kElMaxRadius, HH = kElTileH + 2 * kElMaxRadius;
  __shared__ int16_t sH[HH][HW], sL[HH][HW];       // the tile with its halo: hi, and lo with 32767 where unknown
  __shared__ int16_t rH[HH][kElTileW], rL[HH][kElTileW];      // the row pass
  __shared__ uint32_t red[4];
  const int R = a.radius, k = blockIdx.y;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int x0 = tx * kElTileW, y0 = ty * kElTileH;
  const size_t cells = (size_t)a.mw * a.mh;
  const int16_t* hi = a.hi + (size_t)k * cells;
  const int16_t* lo = a.lo + (size_t)k * cells;
  const int hw = kElTileW + 2 * R, hh = kElTileH + 2 * R;
  for (int e = threadIdx.x; e < hw * hh; e += 256) {
    const int r = e / hw, c = e - r * hw;
    const int gx = x0 - R + c, gy = y0 - R + r;
    int h = kElUnknown, l = 32767;
    if (gx >= 0 && gx < a.mw && gy >= 0 && gy < a.mh) {
      const size_t at = (size_t)gy * a.mw + gx;
      h = hi[at];
      if (h != kElUnknown) l = lo[at];
    }
    sH[r][c] = (int16_t)h, sL[r][c] = (int16_t)l;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < hh * kElTileW; e += 256) {
    const int r = e / kElTileW, c = e - r * kElTileW;
    int mx = kElUnknown, mn = 32767;
    for (int d = 0; d <= 2 * R; ++d) mx = max(mx, (int)sH[r][c + d]), mn = min(mn, (int)sL[r][c + d]);
    rH[r][c] = (int16_t)mx, rL[r][c] = (int16_t)mn;
  }
  __syncthreads();
  const int c = threadIdx.x & 63, gx = x0 + c;
  uint32_t lethal = 0;
#pragma unroll
  for (int e = 0; e < kElTileH / 4; ++e) {
    const int r = (threadIdx.x >> 6) * (kElTileH / 4) + e, gy = y0 + r;
    if (gx >= a.mw || gy >= a.mh) continue;
    const int hc = sH[r + R][c + R], lc = sL[r + R][c + R];
    int t = -1, rise = 0;
    if (hc != kElUnknown) {
      int mx = kElUnknown, mn = 32767;
      for (int d = 0; d <= 2 * R; ++d) mx = max(mx, (int)rH[r + d][c]), mn = min(mn, (int)rL[r + d][c]);
      rise = max(mx - lc, hc - mn);
      t = rise > a.max_step ? 100 : 0;
      lethal += t == 100;
    }
    const size_t at = (size_t)k * cells + (size_t)gy * a.mw + gx;
    if (a.trav) a.trav[at] = (int8_t)t;
    if (a.rise) a.rise[at] = (uint16_t)min(rise, 65535);
  }
  if (a.stats) {
    const uint32_t total = pc_block_sum(lethal, red);
    if (threadIdx.x == 0 && total) atomicAdd(a.stats + (size_t)k * 4 + 1, total);
  }
}

}  // namespace sn
