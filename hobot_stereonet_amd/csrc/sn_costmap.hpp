// sn_costmap.hpp — rolling log-odds costmap with ray clearing, one int16 map per stream (sn_costmap_push; the contract is in
// include/stereonet_hip.h, the numpy twin is hobot_stereonet_amd/costmap.py).  Everything per cell is integer apart from the
// double products of the sector test and of Rb, each rounded once (no FMA).
//
//   k_costmap     grid (slot chunks, streams present in the launch), 256 threads.  The host sorts the launch's maps by stream as
//                 sn_temporal_push does (CmArgs::first / map).  A lane owns ONE slot (i, j) of one stream's torus and walks that
//                 stream's frames with L in a register: the state is read once before the first frame (not at all for a fresh
//                 stream: "all unknown" is the host's flag, so a reset needs no memset) and written once after the last, and
//                 two workgroups never touch the same state word.
//                 Tables in LDS: E (the beam edges as float, staged once per workgroup) and Rb (the frame's returns in subs as
//                 int32, staged once per workgroup and frame).  Steps 2-4 of the contract are per-lane integer work; a cell
//                 with bx <= 0 or outside the sector skips the search, which is at most 12 steps in LDS.
//                 Only the fold of L runs from frame to frame; what a slot sees of a frame (cm_view: its world cell, its base-
//                 frame centre, the grid's word) and the frame's Rb depend on the inputs alone.  So the loop is one stage
//                 ahead: while frame f is folded, the grid word and the first 256 returns of frame f + 1 are in flight, and
//                 Rb has two tables that alternate, which leaves one barrier a frame.
//                 The unrolled outputs: slot (i, j) goes to element [(j - oy) mod mh][(i - ox) mod mw], so consecutive lanes
//                 store consecutive elements except at the wrap column.
//                 Traffic per cell: 2 + 2 bytes of state per launch; per frame grid 1 + logodds 2 where wanted, and at most one
//                 byte of occ (L2-resident: the observation grid is read by many cells' neighbours).
//                 stats: sn_streams.hpp's stats_*.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sn_obstacles.hpp"      // kObMaxBeams, kObMaxCells
#include "sn_streams.hpp"

namespace sn {

constexpr int kCmMaxWindow = 4096;      // mw, mh
constexpr int kCmUnknown = -32768;

struct CmArgs {
  const int8_t* occ;       // [m][gh][gw], or nullptr: no grid observation
  const float* ranges;     // [m][beams], or nullptr: no rays
  const float* edges;      // [beams + 1] (rays only)
  int8_t* grid;            // nullable
  int16_t* logodds;        // nullable
  uint32_t* stats;         // nullable: [m][4], zeroed before the launch
  int16_t* L;              // state [streams][mh][mw]
  double k256;
  long long gx0, gy0, margin, rmin, cmax;
  int mw, mh, gw, gh, beams;
  int l_hit, l_miss, l_min, l_max;
  StreamGroups g;          // the launch's maps, sorted by stream; fresh: all unknown, no previous origin
  TorusPrev t;
  int q[kSlice][6];        // per map of the launch: tx, ty, cq, sq, ox, oy
};

// Rb of the contract: the return of a beam in subs, -1 without one
__device__ __forceinline__ int cm_return_subs(float r, double k256) {
#pragma clang fp contract(off)
  if (!(r > 0.f) || !(r < __builtin_inff())) return -1;
  const double s = floor((double)r * k256);
  return s >= 2147483647.0 ? INT32_MAX : (int)s;
}

// E[i] * bx <= by: one rounded double product
__device__ __forceinline__ bool cm_edge_le(float e, int bx, int by) {
#pragma clang fp contract(off)
  const double prod = (double)e * (double)bx;
  return prod <= (double)by;
}

// what a slot sees in one frame, apart from its own L: where it goes in the unrolled outputs, its world cell, its centre in the
// base frame and the grid's word for it.  None of it depends on the state, so the next frame's is fetched while this one's is used.
struct CmView {
  int ui, uj, cx, cy;
  int bx, by;      // |dx|, |dy| <= (mw/2 + 1) * 256 < 2^20 inside the window, so both fit easily
  int o;
};

__device__ __forceinline__ CmView cm_view(const CmArgs& a, int k, int i, int j) {
  const int* q = a.q[k];
  const int tx = q[0], ty = q[1], cq = q[2], sq = q[3], ox = q[4], oy = q[5];
  CmView v;
  v.ui = torus_unroll(i, torus_mod(ox, a.mw), a.mw), v.uj = torus_unroll(j, torus_mod(oy, a.mh), a.mh);      // the mod of the origin is the wave's, not the lane's
  v.cx = ox + v.ui, v.cy = oy + v.uj;
  // |cx| <= 2^22 + 2^12 and |tx| <= 2^30, so cx*256 + 128 fits in 32 bits and every product below is 32 x 32 -> 64
  const int dx = v.cx * 256 + 128 - tx, dy = v.cy * 256 + 128 - ty;
  v.bx = (int)(((long long)cq * dx + (long long)sq * dy + (1ll << 29)) >> 30);
  v.by = (int)(((long long)cq * dy - (long long)sq * dx + (1ll << 29)) >> 30);
  v.o = -1;
  if (a.occ) {
    const long long qx = ((long long)v.bx - a.gx0) >> 8, qy = ((long long)v.by - a.gy0) >> 8;
    if (qx >= 0 && qx < a.gw && qy >= 0 && qy < a.gh) v.o = a.occ[((size_t)k * a.gh + (size_t)qy) * a.gw + (size_t)qx];
  }
  return v;
}

// grid (ceil(mh*mw / 256), groups); dynamic LDS: (beams + 1) floats, then two tables of beams int32 (this frame's Rb and the next's)
__global__ __launch_bounds__(256) void k_costmap(CmArgs a) {
  extern __shared__ __align__(16) uint32_t cm_lds[];
  __shared__ uint32_t cnt[kSlice][4];
  float* E = reinterpret_cast<float*>(cm_lds);
  int* Rb2 = reinterpret_cast<int*>(cm_lds + a.beams + 1);
  const bool rays = a.ranges != nullptr;
  const int g = blockIdx.y, f0 = a.g.first[g], f1 = a.g.first[g + 1];
  const int cells = a.mw * a.mh;      // <= 2^24
  const int p = blockIdx.x * 256 + threadIdx.x;
  const bool live = p < cells;
  const int j = live ? p / a.mw : 0, i = live ? p - j * a.mw : 0;
  if (a.stats) stats_clear(cnt, f1 - f0);
  if (rays) {
    for (int b = threadIdx.x; b <= a.beams; b += 256) E[b] = a.edges[b];
    for (int b = threadIdx.x; b < a.beams; b += 256) Rb2[b] = cm_return_subs(a.ranges[(size_t)a.g.map[f0] * a.beams + b], a.k256);
  }
  __syncthreads();
  const size_t sp = (size_t)a.g.stream[g] * cells + p;
  bool seen = !a.g.fresh[g];
  int pox = a.t.pox[g], poy = a.t.poy[g];
  int L = kCmUnknown;
  if (live && seen) L = a.L[sp];
  const uint32_t span = (uint32_t)(a.l_max - a.l_min);      // <= 65534, and (L - l_min) * 100 < 2^23
  CmView next = cm_view(a, a.g.map[f0], i, j);
#pragma unroll 1
  for (int f = f0; f < f1; ++f) {
    const int k = a.g.map[f], ox = a.q[k][4], oy = a.q[k][5];
    const CmView v = next;
    const int* Rb = Rb2 + ((f - f0) & 1) * a.beams;
    // the next frame's inputs are asked for before this frame's are used: its first 256 returns and its grid word
    const bool more = f + 1 < f1;
    const int kn = more ? a.g.map[f + 1] : k;
    const float* rn = rays ? a.ranges + (size_t)kn * a.beams : nullptr;
    const float r_first = more && rays && (int)threadIdx.x < a.beams ? rn[threadIdx.x] : 0.f;
    if (more) next = cm_view(a, kn, i, j);
    uint32_t n_known = 0, n_pos = 0, n_hit = 0, n_clear = 0;
    if (live) {
      torus_if_rolled(seen, i, j, v.cx, v.cy, pox, poy, a.mw, a.mh, [&] { L = kCmUnknown; });
      bool ray = false;
      if (rays && v.o != 100 && v.o != 0 && v.bx > 0 && cm_edge_le(E[0], v.bx, v.by) && !cm_edge_le(E[a.beams], v.bx, v.by)) {
        int lo = 0, hi = a.beams;      // E[lo]*bx <= by, not E[hi]*bx <= by
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (cm_edge_le(E[mid], v.bx, v.by)) lo = mid;
          else hi = mid;
        }
        const long long R = Rb[lo], C = R - a.margin, r2 = (long long)v.bx * v.bx + (long long)v.by * v.by;
        ray = R >= 0 && C > 0 && r2 < C * C && r2 >= a.rmin * a.rmin && (a.cmax == 0 || r2 <= a.cmax * a.cmax);
      }
      const int L0 = L == kCmUnknown ? 0 : L;
      if (v.o == 100) {
        L = min(L0 + a.l_hit, a.l_max);
        n_hit = 1;
      } else if (v.o == 0 || ray) {
        L = max(L0 - a.l_miss, a.l_min);
        n_clear = 1;
      }
      n_known = L != kCmUnknown, n_pos = L > 0;
      const size_t op = (size_t)k * cells + (size_t)v.uj * a.mw + v.ui;
      if (a.grid) a.grid[op] = L == kCmUnknown ? (int8_t)-1 : (int8_t)(((uint32_t)(L - a.l_min) * 100u + span / 2) / span);
      if (a.logodds) a.logodds[op] = (int16_t)L;
    }
    seen = true, pox = ox, poy = oy;
    if (a.stats) stats_frame(cnt[f - f0], n_known | (n_pos << 16), n_hit | (n_clear << 16));      // wave-uniform; a wave's sums are at most 64
    if (more && rays) {      // the other table: nobody reads it in this frame, and the barrier hands it to the next
      int* Rn = Rb2 + ((f + 1 - f0) & 1) * a.beams;
      if ((int)threadIdx.x < a.beams) Rn[threadIdx.x] = cm_return_subs(r_first, a.k256);
      for (int b = threadIdx.x + 256; b < a.beams; b += 256) Rn[b] = cm_return_subs(rn[b], a.k256);
      __syncthreads();
    }
  }
  if (live && f1 > f0) a.L[sp] = (int16_t)L;
  if (a.stats) stats_flush(cnt, a.stats, a.g.map, f0, f1);
}

}  // namespace sn
