// sn_obstacles.hpp — int32 disparity map -> bird's-eye obstacle grid and laser scan (sn_obstacles_from_raw,
// include/stereonet_hip.h).  A scatter with collisions whose every accumulator is an integer (a count, a maximum of
// millimetres, a minimum of the bits of a positive float), so the result does not depend on the order of arrival and equals
// the numpy twin's (hobot_stereonet_amd/obstacles.py) byte for byte.
//   k_ob_fill         one launch starts every accumulator: hits and stats = 0, height_mm = INT32_MIN, ranges = +inf.
//   k_ob_accumulate   the hot path: per sample a 4-byte raw read; X, Y, Z and valid through the point cloud's device functions
//                     (pc_depth, pc_valid, pc_point), the base frame, the class, the cell and the beam.  A lane owns one
//                     output column and walks the rows of its workgroup's chunk, so consecutive lanes read consecutive words.
//                     RLE form: the lane keeps its current cell (two counts, the maximum height) and its current beam (the
//                     minimum range, the beam's two edges) in registers and sends them when the cell or the beam changes: a
//                     wall fills one cell and one beam from a whole column, far ground one cell from many rows.  The lanes
//                     of a wave that leave their cells at the same row, and what the lanes hold at the end of the walk, are
//                     summed over the wave's runs of equal cells first (ob_wave_flush): one set of atomics per run.
//                     The ranges row is accumulated in LDS and flushed once per workgroup, finite entries only.
//                     MOUNTS (sn_obstacles_from_raw_mounts): a second instantiation reads the map's mount from memory.
//                     Plain form (SN_OBSTACLE_RLE=0): the same arithmetic, one set of global atomics per point.
//   k_ob_classify     a pass over the cells: occ from the two counts and the thresholds, stats from block sums, one integer
//                     atomic per workgroup and statistic (as k_pc_organised's count).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "sn_pointcloud.hpp"

namespace sn {

constexpr int kObMaxCells = 4096;      // gw, gh
constexpr int kObMaxBeams = 4096;
constexpr int kObAhead = 4;            // rows a lane loads before it works on them
constexpr uint32_t kObInf = 0x7f800000u;

struct ObArgs {
  PcArgs pc;              // raw, W, H, Wo, Ho, step, scale, fB, fx, fy, cx, cy, zmin, zmax: the point cloud's sample arithmetic
  const float* edges;     // [beams + 1] (scan only)
  uint32_t* hits;         // [n][gh][gw][2], or nullptr: no grid
  int32_t* height;        // [n][gh][gw], nullable
  uint32_t* ranges;       // [n][beams] as bits, or nullptr: no scan
  float m[12];
  const float* mounts;    // MOUNTS: map k's mount is the twelve floats at mounts + k * mount_stride, and m is not used
  int mount_stride;
  float x_min, y_min, cell, z_floor, z_lo, z_hi, r_min, r_max;
  int gw, gh, beams;
  int chunks, rows;       // row chunks per column block, output rows per chunk
};

struct ObClassArgs {
  const uint32_t* hits;   // [n][cells][2]
  int8_t* occ;            // [n][cells], nullable
  uint32_t* stats;        // [n][4], nullable
  int cells, min_obstacle, min_ground;
};

// edges[i] = (float)tan(angle_min + i * angle_increment) in double, i = 0..beams; false unless 1 <= beams <= kObMaxBeams, the
// sector lies inside (-pi/2, pi/2) and the rounded edges increase strictly
inline bool ob_beam_edges(int beams, float angle_min, float angle_increment, float* edges) {
  if (beams < 1 || beams > kObMaxBeams || !std::isfinite(angle_min) || !std::isfinite(angle_increment)) return false;
  const double half_pi = 1.57079632679489661923;
  for (int i = 0; i <= beams; ++i) {
    const double a = (double)angle_min + (double)i * (double)angle_increment;
    if (!(a > -half_pi && a < half_pi)) return false;
    edges[i] = (float)std::tan(a);
    if (i && !(edges[i] > edges[i - 1])) return false;
  }
  return true;
}

// p_base = R p_cam + t, left to right, every operation rounded
__device__ __forceinline__ float ob_row(const float* m, float x, float y, float z) {
#pragma clang fp contract(off)
  return ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
}

// the cell index iy * gw + ix of (xb, yb), or -1 outside the grid: tested in float before the conversion
__device__ __forceinline__ int ob_cell(const ObArgs& a, float xb, float yb) {
#pragma clang fp contract(off)
  const float qx = floorf((xb - a.x_min) / a.cell), qy = floorf((yb - a.y_min) / a.cell);
  if (!(qx >= 0.f && qx < (float)a.gw && qy >= 0.f && qy < (float)a.gh)) return -1;
  return (int)qy * a.gw + (int)qx;
}

// (int)floorf(zb * 1000), saturated to int32 as the hardware's conversion does
__device__ __forceinline__ int ob_height_mm(float zb) {
#pragma clang fp contract(off)
  const float f = floorf(zb * 1000.f);
  return f >= 2147483648.f ? INT32_MAX : (f <= -2147483648.f ? INT32_MIN : (int)f);
}

__device__ __forceinline__ float ob_range(float xb, float yb) {
#pragma clang fp contract(off)
  const float xx = xb * xb, yy = yb * yb;
  return sqrtf(xx + yy);
}

// the number of edges <= t, minus 1, for edges[0] <= t < edges[beams]
__device__ __forceinline__ int ob_beam(const float* edges, int beams, float t) {
  int lo = 0, hi = beams;      // edges[lo] <= t < edges[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (edges[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

// one launch starts every accumulator: `zeros` words of 0 (hits, then stats where both are wanted: see the entry point), height_mm
// = INT32_MIN, ranges = +inf
struct ObFillArgs {
  uint32_t* hits;
  uint32_t* stats;
  int32_t* height;
  uint32_t* ranges;
  size_t n_hits, n_stats, n_height, n_ranges;      // words
};

__global__ __launch_bounds__(256) void k_ob_fill(ObFillArgs a) {
  const size_t e1 = a.n_hits, e2 = e1 + a.n_stats, e3 = e2 + a.n_height, e4 = e3 + a.n_ranges;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < e4; i += (size_t)gridDim.x * 256) {
    if (i < e1) a.hits[i] = 0u;
    else if (i < e2) a.stats[i - e1] = 0u;
    else if (i < e3) a.height[i - e2] = INT32_MIN;
    else a.ranges[i - e3] = kObInf;
  }
}

// A flush by the whole wave: neighbouring columns are mostly in the same cell, so every run of lanes with one cell is summed
// with shuffles and its first lane sends the atomics.  cur < 0: the lane has nothing to send.
__device__ __forceinline__ void ob_wave_flush(int cur, uint32_t n_ob, uint32_t n_gr, int hmax, uint32_t* hits, int32_t* height) {
  const int lane = threadIdx.x & 63;
  const int before = __shfl_up(cur, 1);
  const bool head = lane == 0 || before != cur;
  const int run = __popcll(__ballot(head) & (~0ull >> (63 - lane)));      // the runs are numbered, so equal numbers are contiguous
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int run_o = __shfl_down(run, o), h_o = __shfl_down(hmax, o);
    const uint32_t ob_o = __shfl_down(n_ob, o), gr_o = __shfl_down(n_gr, o);
    if (lane + o < 64 && run_o == run) n_ob += ob_o, n_gr += gr_o, hmax = max(hmax, h_o);
  }
  if (!head || cur < 0) return;
  if (n_ob) atomicAdd(hits + 2 * (size_t)cur, n_ob);
  if (n_gr) atomicAdd(hits + 2 * (size_t)cur + 1, n_gr);
  if (height && n_ob) atomicMax(height + cur, hmax);
}

// grid (column blocks * chunks, n), 256 lanes = 256 output columns; dynamic LDS: (beams + 1) floats [+ beams words, RLE]
template <bool RLE, bool MOUNTS>
__global__ __launch_bounds__(256) void k_ob_accumulate(ObArgs a) {
  extern __shared__ __align__(16) uint32_t ob_lds[];
  const bool grid = a.hits != nullptr, scan = a.ranges != nullptr;
  float* edges = reinterpret_cast<float*>(ob_lds);
  uint32_t* lds_near = ob_lds + a.beams + 1;      // RLE: this workgroup's copy of the ranges row
  const int k = blockIdx.y;
  float own[12];      // MOUNTS: the map's mount, the same for every lane
  if (MOUNTS) {
#pragma unroll
    for (int e = 0; e < 12; ++e) own[e] = a.mounts[(size_t)k * a.mount_stride + e];
  }
  const float* m = MOUNTS ? own : a.m;
  uint32_t* g_ranges = scan ? a.ranges + (size_t)k * a.beams : nullptr;
  if (scan) {
    for (int b = threadIdx.x; b <= a.beams; b += 256) edges[b] = a.edges[b];
    if (RLE)
      for (int b = threadIdx.x; b < a.beams; b += 256) lds_near[b] = kObInf;
    __syncthreads();
  }
  const int cblock = blockIdx.x / a.chunks, chunk = blockIdx.x - cblock * a.chunks;
  const int j = cblock * 256 + threadIdx.x, u = j * a.pc.step;
  const int i0 = chunk * a.rows, i1 = min(i0 + a.rows, a.pc.Ho);
  const size_t cells = (size_t)a.gw * a.gh;
  uint32_t* hits = grid ? a.hits + (size_t)k * cells * 2 : nullptr;
  int32_t* height = a.height ? a.height + (size_t)k * cells : nullptr;
  const float e_first = scan ? edges[0] : 0.f, e_last = scan ? edges[a.beams] : 0.f;

  // the lane's run: the cell it is in, with what it has seen of it, and the beam
  int cur = -1, hmax = INT32_MIN, beam = -1;
  uint32_t n_ob = 0, n_gr = 0, rmin = kObInf;
  float b_lo = 0.f, b_hi = 0.f;
  auto flush_cell = [&]() {
    if (cur < 0) return;
    if (n_ob) atomicAdd(hits + 2 * (size_t)cur, n_ob);
    if (n_gr) atomicAdd(hits + 2 * (size_t)cur + 1, n_gr);
    if (height && n_ob) atomicMax(height + cur, hmax);
  };
  auto flush_beam = [&]() {
    if (beam >= 0) atomicMin(RLE ? lds_near + beam : g_ranges + beam, rmin);
  };

  // Every lane of the wave walks the same rows (a column beyond Wo reads nothing), so the wave meets at one point per row: where
  // any lane leaves its cell, the leaving lanes flush together (ob_wave_flush) — on the ground a row of lanes leaves together.
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
      bool ground = false, obstacle = false;
      float xb = 0.f, yb = 0.f, zb = 0.f;
      int c = -1;
      if (pc_valid(r[e], z, a.pc)) {
        const float4 p = pc_point<false>(a.pc, nullptr, u, (ib + e) * a.pc.step, z);
        zb = ob_row(m + 8, p.x, p.y, p.z);
        ground = a.z_floor <= zb && zb <= a.z_lo, obstacle = a.z_lo < zb && zb <= a.z_hi;
        if (ground || obstacle) {
          xb = ob_row(m, p.x, p.y, p.z), yb = ob_row(m + 4, p.x, p.y, p.z);
          if (grid) c = ob_cell(a, xb, yb);
        }
      }
      if (RLE && grid) {
        const bool leaves = c >= 0 && cur >= 0 && c != cur;
        if (__any(leaves)) {
          ob_wave_flush(leaves ? cur : -1, n_ob, n_gr, hmax, hits, height);
          if (leaves) cur = -1;
        }
      }
      if (c >= 0) {
        if (c != cur) cur = c, n_ob = n_gr = 0, hmax = INT32_MIN;
        if (obstacle) {
          ++n_ob;
          hmax = max(hmax, ob_height_mm(zb));
        } else {
          ++n_gr;
        }
        if (!RLE) {
          flush_cell();
          cur = -1;
        }
      }
      if (scan && obstacle && xb > 0.f) {
        const float t = yb / xb;
        if (e_first <= t && t < e_last) {
          const float rr = ob_range(xb, yb);
          if (a.r_min <= rr && rr <= a.r_max) {
            if (!(beam >= 0 && b_lo <= t && t < b_hi)) {
              flush_beam();
              beam = ob_beam(edges, a.beams, t);
              b_lo = edges[beam], b_hi = edges[beam + 1], rmin = kObInf;
            }
            rmin = min(rmin, __float_as_uint(rr));
            if (!RLE) {
              flush_beam();
              beam = -1;
            }
          }
        }
      }
    }
  }
  flush_beam();
  if (RLE && grid) ob_wave_flush(cur, n_ob, n_gr, hmax, hits, height);      // every lane of the wave, its columns beyond Wo included
  if (RLE && scan) {
    __syncthreads();
    for (int b = threadIdx.x; b < a.beams; b += 256)
      if (lds_near[b] != kObInf) atomicMin(g_ranges + b, lds_near[b]);
  }
}

// grid (workgroups per map, n)
__global__ __launch_bounds__(256) void k_ob_classify(ObClassArgs a) {
  __shared__ uint32_t red[4];
  const int k = blockIdx.y;
  const uint32_t* hits = a.hits + (size_t)k * a.cells * 2;
  uint32_t s[4] = {0, 0, 0, 0};      // obstacle points, ground points, occupied cells, free cells
  for (int c = blockIdx.x * 256 + threadIdx.x; c < a.cells; c += gridDim.x * 256) {
    const uint32_t ob = hits[2 * (size_t)c], gr = hits[2 * (size_t)c + 1];
    const bool occupied = ob >= (uint32_t)a.min_obstacle, free_ = !occupied && gr >= (uint32_t)a.min_ground;
    if (a.occ) a.occ[(size_t)k * a.cells + c] = occupied ? 100 : (free_ ? 0 : -1);
    s[0] += ob, s[1] += gr, s[2] += occupied, s[3] += free_;
  }
  if (!a.stats) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t total = pc_block_sum(s[q], red);
    if (threadIdx.x == 0 && total) atomicAdd(a.stats + 4 * k + q, total);
  }
}

}  // namespace sn
