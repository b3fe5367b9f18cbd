// sn_pointcloud.hpp — int32 disparity map -> 3-D points {X, Y, Z, rgb} (sn_pointcloud_from_raw, include/stereonet_hip.h).
//
// Memory-bound: per sample a 4-byte raw read (plus 1.5 NV12 bytes with colour) and a 16-byte point write.
//   k_pc_organised  one wave = 256 output columns of one row, one float4 store per point and lane so that every store
//                   instruction writes 1 KiB of contiguous points (int4 raw loads at step 1, transposed through LDS);
//                   the per-map valid count is one integer atomicAdd per workgroup (order-free).
//   k_pc_count      compact form, pass 1: a workgroup counts the valid samples of one tile of kPcTile samples of one map
//                   (64-bit ballot + popcount per wave, wave totals through LDS) -> scratch[k][t].
//   k_pc_write      pass 2: sums scratch[k][0..t) itself, recomputes validity, ranks each valid lane (mbcnt over the
//                   ballot + exclusive scan of the wave totals) and writes at base + rank: raster order, deterministic,
//                   no atomics.  The last tile's workgroup writes counts[k].
// The depth is k_depth_from_raw's float / double mix (Parse, parser.cpp:84-86) so that Z is bit-identical to it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sn {

constexpr int kPcIters = 16;                 // 64-sample ballots per wave per tile
constexpr int kPcTile = 4 * 64 * kPcIters;   // samples per compact tile (4 waves); never straddles maps

struct PcArgs {
  const int32_t* raw;       // [n][H][W]
  const uint8_t* nv12;      // [n] frames of nv12_frame bytes, or nullptr (no colour)
  float4* pts;              // [n][Ho * Wo]
  uint32_t* counts;         // [n] (nullable in the organised form)
  uint32_t* scratch;        // compact: [n][tiles] valid samples per tile
  size_t nv12_frame;        // bytes per NV12 frame
  int W, H, Wo, Ho, step, pitch, tiles;
  float scale, fB, fx, fy, cx, cy, zmin, zmax;
  int vec;                  // organised: raw rows are read as int4 (step 1, W % 4 == 0, raw 16-byte aligned)
};

__device__ __forceinline__ float pc_depth(int32_t r, float scale, float fB) {
  const float dis = (float)r * scale;
  return (float)((double)fB / ((double)dis * 16.0 * 12.0) / 1000.0);
}

// Parse's arithmetic per element (parser.cpp:84-86): the product f * B is a float, everything after it is double
__global__ __launch_bounds__(256) void k_depth_from_raw(const int32_t* __restrict__ raw, size_t n, float scale, float fB,
                                                        float* __restrict__ depth, float* __restrict__ disp) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float dis = (float)raw[i] * scale;
    depth[i] = (float)((double)fB / ((double)dis * 16.0 * 12.0) / 1000.0);
    if (disp) disp[i] = dis * 16.0f * 12.0f;
  }
}

__device__ __forceinline__ bool pc_valid(int32_t r, float z, const PcArgs& a) {
  return r > 0 && a.zmin <= z && (a.zmax <= 0.f || z <= a.zmax);
}

__device__ __forceinline__ int pc_clamp255(int x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }

// JFIF full-range BT.601 in integers, true NV12 chroma siting: 0x00RRGGBB
__device__ __forceinline__ uint32_t pc_rgb(const uint8_t* __restrict__ f, int pitch, int H, int u, int v) {
  const int y = f[(size_t)v * pitch + u];
  const uint8_t* uv = f + (size_t)pitch * H + (size_t)(v >> 1) * pitch + (u & ~1);
  const int uc = (int)uv[0] - 128, vc = (int)uv[1] - 128;
  const int r = pc_clamp255(y + ((91881 * vc + 32768) >> 16));
  const int g = pc_clamp255(y + ((-22554 * uc - 46802 * vc + 32768) >> 16));
  const int b = pc_clamp255(y + ((116130 * uc + 32768) >> 16));
  return ((uint32_t)r << 16) | ((uint32_t)g << 8) | (uint32_t)b;
}

template <bool COLOUR>
__device__ __forceinline__ float4 pc_point(const PcArgs& a, const uint8_t* frame, int u, int v, float z) {
  const float x = ((float)u - a.cx) * z / a.fx;
  const float y = ((float)v - a.cy) * z / a.fy;
  const uint32_t rgb = COLOUR ? pc_rgb(frame, a.pitch, a.H, u, v) : 0u;
  return make_float4(x, y, z, __uint_as_float(rgb));
}

// sum of one value per thread over the 256-thread workgroup (every thread gets it); lds: 4 words
__device__ __forceinline__ uint32_t pc_block_sum(uint32_t v, uint32_t* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return lds[0] + lds[1] + lds[2] + lds[3];
}

// grid (workgroups per map, n); each wave takes one segment of 256 output columns of one row of map blockIdx.y per
// iteration (grid-stride over (row, segment), uniform across the workgroup).  Lane l handles columns seg + e*64 + l,
// e = 0..3, so every float4 store instruction of a wave writes 1 KiB of contiguous points.  At step 1 (a.vec) the raw
// row is read as one int4 per lane (columns seg + 4l .. +3) and transposed through LDS into that order.
template <bool COLOUR>
__global__ __launch_bounds__(256) void k_pc_organised(PcArgs a) {
  __shared__ int4 tr[4][64];
  __shared__ uint32_t red[4];
  const int k = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int spr = (a.Wo + 255) >> 8, nseg = a.Ho * spr;
  const int32_t* raw = a.raw + (size_t)k * a.H * a.W;
  const uint8_t* frame = COLOUR ? a.nv12 + (size_t)k * a.nv12_frame : nullptr;
  float4* out = a.pts + (size_t)k * a.Ho * a.Wo;
  const float nan = __uint_as_float(0x7fc00000u);
  uint32_t cnt = 0;
  for (int base = blockIdx.x * 4; base < nseg; base += gridDim.x * 4) {
    const int seg = base + wave;
    const bool live = seg < nseg;
    const int i = live ? seg / spr : 0, cb = (seg - i * spr) * 256, v = i * a.step;
    const int32_t* row = raw + (size_t)v * a.W;
    int r[4];
    if (a.vec) {
      __syncthreads();                                   // the previous iteration's reads of tr are done
      if (live && cb + 4 * lane < a.Wo) tr[wave][lane] = *reinterpret_cast<const int4*>(row + cb + 4 * lane);
      __syncthreads();
      const int* t = reinterpret_cast<const int*>(tr[wave]);
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = t[e * 64 + lane];   // stale beyond Wo: never used
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = cb + e * 64 + lane;
        r[e] = live && j < a.Wo ? row[(size_t)j * a.step] : 0;
      }
    }
    if (!live) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = cb + e * 64 + lane;
      if (j >= a.Wo) break;
      const float z = pc_depth(r[e], a.scale, a.fB);
      if (pc_valid(r[e], z, a)) {
        out[(size_t)i * a.Wo + j] = pc_point<COLOUR>(a, frame, j * a.step, v, z);
        ++cnt;
      } else {
        out[(size_t)i * a.Wo + j] = make_float4(nan, nan, nan, 0.f);
      }
    }
  }
  if (a.counts) {
    const uint32_t total = pc_block_sum(cnt, red);
    if (threadIdx.x == 0 && total) atomicAdd(a.counts + k, total);
  }
}

// The validity pass of one compact tile: wave w covers samples [t*kPcTile + w*1024, +1024) of map k in kPcIters ballots of
// 64 consecutive samples; returns the wave's valid count, z[] / m[] hold each lane's depth and each ballot.
__device__ __forceinline__ uint32_t pc_tile_masks(const PcArgs& a, int k, int t, float (&z)[kPcIters],
                                                  unsigned long long (&m)[kPcIters]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_out = a.Ho * a.Wo;
  const int p0 = t * kPcTile + wave * (64 * kPcIters) + lane;
  const int32_t* raw = a.raw + (size_t)k * a.H * a.W;
  int i = p0 / a.Wo, j = p0 - i * a.Wo;
  uint32_t total = 0;
#pragma unroll
  for (int it = 0; it < kPcIters; ++it) {
    const bool in = p0 + it * 64 < n_out;
    const int32_t r = in ? raw[(size_t)i * a.step * a.W + j * a.step] : 0;
    z[it] = pc_depth(r, a.scale, a.fB);
    m[it] = __ballot(in && pc_valid(r, z[it], a));
    total += (uint32_t)__popcll(m[it]);
    for (j += 64; j >= a.Wo; j -= a.Wo) ++i;
  }
  return total;
}

// grid (tiles, n)
__global__ __launch_bounds__(256) void k_pc_count(PcArgs a) {
  __shared__ uint32_t red[4];
  float z[kPcIters];
  unsigned long long m[kPcIters];
  const int k = blockIdx.y, t = blockIdx.x;
  const uint32_t wave_total = pc_tile_masks(a, k, t, z, m);
  const uint32_t total = pc_block_sum((threadIdx.x & 63) == 0 ? wave_total : 0u, red);
  if (threadIdx.x == 0) a.scratch[(size_t)k * a.tiles + t] = total;
}

// grid (tiles, n)
template <bool COLOUR>
__global__ __launch_bounds__(256) void k_pc_write(PcArgs a) {
  __shared__ uint32_t red[4], wtot[4];
  float z[kPcIters];
  unsigned long long m[kPcIters];
  const int k = blockIdx.y, t = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t before = 0;       // valid samples of map k in the tiles before this one
  for (int q = threadIdx.x; q < t; q += 256) before += a.scratch[(size_t)k * a.tiles + q];
  before = pc_block_sum(before, red);
  const uint32_t wave_total = pc_tile_masks(a, k, t, z, m);
  if (lane == 0) wtot[wave] = wave_total;
  __syncthreads();
  uint32_t rank = before;
  for (int w = 0; w < wave; ++w) rank += wtot[w];
  if (t == a.tiles - 1 && threadIdx.x == 0) a.counts[k] = before + wtot[0] + wtot[1] + wtot[2] + wtot[3];
  const uint8_t* frame = COLOUR ? a.nv12 + (size_t)k * a.nv12_frame : nullptr;
  float4* out = a.pts + (size_t)k * a.Ho * a.Wo;
  const int p0 = t * kPcTile + wave * (64 * kPcIters) + lane;
  int i = p0 / a.Wo, j = p0 - i * a.Wo;
#pragma unroll
  for (int it = 0; it < kPcIters; ++it) {
    if ((m[it] >> lane) & 1ull) {
      const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m[it] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m[it], 0u));
      out[rank + below] = pc_point<COLOUR>(a, frame, j * a.step, i * a.step, z[it]);
    }
    rank += (uint32_t)__popcll(m[it]);
    for (j += 64; j >= a.Wo; j -= a.Wo) ++i;
  }
}

}  // namespace sn
