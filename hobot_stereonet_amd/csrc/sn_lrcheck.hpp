// sn_lrcheck.hpp — left-right consistency check of two int32 disparity maps and the eye-swapping mirror of the model input
// (sn_mirror_pair_i8, sn_lr_check, sn_infer_lrc; the contract is in include/stereonet_hip.h).
//
// Both kernels are memory-bound.
//   k_mirror_pair  out[k][c][v][u] = in[k][(c + 3) % 6][v][W - 1 - u]: 12 bytes of traffic per pixel and pair.  VEC (W % 16 == 0,
//                  16-byte aligned tensors): one thread moves one 16-byte chunk — dwordx4 load of the source row's chunk
//                  cpr - 1 - j, bytes reversed in registers (bswap per word + word swap), dwordx4 store of chunk j, so a wave
//                  stores 1 KiB of contiguous bytes per instruction and reads the 1 KiB that mirrors it.  Any other width
//                  (1242: rows are not even 4-byte aligned) moves one byte per thread.
//   k_lr_check     one wave = 256 consecutive columns of one row per iteration.  VEC (W % 4 == 0, aligned maps): one int4 of the
//                  left map per lane, one int4 store of the masked map, one dword of four mask bytes.  Otherwise lane l takes
//                  columns seg + e*64 + l.  The partner samples R(x0), R(x0 + 1) are gathered straight from global memory: the
//                  lanes of a wave walk the right row monotonically (u - d with a smooth d), so one gather instruction touches a
//                  handful of neighbouring 128-byte lines that the CU's 32 KiB L1 and the L2 hold (a row is <= 5 KiB and every
//                  line is fetched from HBM once).  An LDS window was not built: the contract bounds the disparity by nothing
//                  (raw is any int32), so a staged window [u0 - dmax, u0 + 256) would still need this path as its fallback,
//                  and it would add a barrier per segment to save traffic that never leaves the caches.
//                  kept[k]: per-thread integer counts, one atomicAdd per workgroup (integer, order-free).
// The arithmetic is fp32 with every operation rounded on its own: lrc_reason turns the compiler's contraction off (hipcc's
// default would fuse u - rl*S, d0 + t*(d1 - d0) and tau_px + tau_rel*d into FMAs; the ISA must show v_mul / v_sub / v_add
// and no v_fma), so the kernel equals the numpy twin (hobot_stereonet_amd/lrcheck.py) bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sn_pointcloud.hpp"   // pc_block_sum
#include "../../include/stereonet_hip.h"   // SN_LRC_*

namespace sn {

struct MirrorArgs {
  const int8_t* in;    // [n][6][H][W]
  int8_t* out;         // [n][6][H][W], no overlap with in
  int n, H, W;
};

__device__ __forceinline__ size_t mirror_src_row(const MirrorArgs& a, size_t row) {     // row = (k*6 + c)*H + v
  const size_t plane = row / a.H, v = row - plane * a.H;
  const size_t k = plane / 6, c = plane - k * 6;
  return (k * 6 + (c + 3) % 6) * a.H + v;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_mirror_pair(MirrorArgs a) {
  const size_t rows = (size_t)a.n * 6 * a.H;
  if (VEC) {
    const size_t cpr = (size_t)a.W >> 4, total = rows * cpr;
    const uint4* src = reinterpret_cast<const uint4*>(a.in);
    uint4* dst = reinterpret_cast<uint4*>(a.out);
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (size_t)gridDim.x * 256) {
      const size_t row = g / cpr, j = g - row * cpr;
      const uint4 x = src[mirror_src_row(a, row) * cpr + (cpr - 1 - j)];
      dst[g] = make_uint4(__builtin_bswap32(x.w), __builtin_bswap32(x.z), __builtin_bswap32(x.y), __builtin_bswap32(x.x));
    }
  } else {
    const size_t W = (size_t)a.W, total = rows * W;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (size_t)gridDim.x * 256) {
      const size_t row = g / W, u = g - row * W;
      a.out[g] = a.in[mirror_src_row(a, row) * W + (W - 1 - u)];
    }
  }
}

struct LrcArgs {
  const int32_t* left;     // [n][H][W]
  const int32_t* right;    // [n][H][W], column-reversed when `mirrored`
  int32_t* out_raw;        // nullable; may be `left`
  float* disp;             // nullable: 0.0f is written at the rejected pixels only
  uint8_t* mask;           // nullable: SN_LRC_* reason per pixel
  uint32_t* kept;          // nullable: [n], zeroed before the launch
  int32_t* right_out;      // nullable: the right map in right-image coordinates
  int W, H;
  float S, tau_px, tau_rel;
  int mirrored;
};

__device__ __forceinline__ int32_t lrc_right(const LrcArgs& a, const int32_t* __restrict__ rrow, int x) {
  return rrow[a.mirrored ? a.W - 1 - x : x];
}

// the contract of sn_lr_check for one pixel: the reason it is rejected for, SN_LRC_KEPT if it is not
__device__ __forceinline__ uint32_t lrc_reason(const LrcArgs& a, const int32_t* __restrict__ rrow, int u, int32_t rl) {
#pragma clang fp contract(off)
  if (rl <= 0) return SN_LRC_INVALID_IN;
  const float d = (float)rl * a.S;
  const float xr = (float)u - d;
  if (xr < 0.f) return SN_LRC_OUT_OF_VIEW;
  const int x0 = (int)floorf(xr);               // 0 <= xr <= u, so 0 <= x0 <= W - 1
  const float t = xr - (float)x0;
  const int x1 = min(x0 + 1, a.W - 1);
  const int32_t r0 = lrc_right(a, rrow, x0), r1 = lrc_right(a, rrow, x1);
  const float d0 = (float)r0 * a.S, d1 = (float)r1 * a.S;
  float dr;
  if (r0 <= 0 && r1 <= 0) return SN_LRC_NO_PARTNER;
  if (r0 <= 0) dr = d1;
  else if (r1 <= 0) dr = d0;
  else dr = d0 + t * (d1 - d0);
  const float tol = a.tau_px + a.tau_rel * d;
  return fabsf(d - dr) <= tol ? SN_LRC_KEPT : SN_LRC_INCONSISTENT;
}

// grid (workgroups per map, n); each wave takes one segment of 256 columns of one row of map blockIdx.y per iteration
template <bool VEC>
__global__ __launch_bounds__(256) void k_lr_check(LrcArgs a) {
  __shared__ uint32_t red[4];
  const int k = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int spr = (a.W + 255) >> 8, nseg = a.H * spr;
  uint32_t cnt = 0;
  for (int seg = blockIdx.x * 4 + wave; seg < nseg; seg += gridDim.x * 4) {
    const int v = seg / spr, cb = (seg - v * spr) * 256;
    const size_t row = ((size_t)k * a.H + v) * a.W;
    const int32_t* rrow = a.right + row;
    if (VEC) {
      const int u0 = cb + 4 * lane;
      if (u0 >= a.W) continue;
      const int4 l = *reinterpret_cast<const int4*>(a.left + row + u0);
      const int32_t rl[4] = {l.x, l.y, l.z, l.w};
      uint32_t m[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        m[e] = lrc_reason(a, rrow, u0 + e, rl[e]);
        cnt += m[e] == SN_LRC_KEPT;
      }
      if (a.out_raw)
        *reinterpret_cast<int4*>(a.out_raw + row + u0) = make_int4(m[0] ? 0 : rl[0], m[1] ? 0 : rl[1], m[2] ? 0 : rl[2], m[3] ? 0 : rl[3]);
      if (a.mask) *reinterpret_cast<uint32_t*>(a.mask + row + u0) = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
      if (a.disp) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (m[e]) a.disp[row + u0 + e] = 0.f;
      }
      if (a.right_out)
        *reinterpret_cast<int4*>(a.right_out + row + u0) =
            make_int4(lrc_right(a, rrow, u0), lrc_right(a, rrow, u0 + 1), lrc_right(a, rrow, u0 + 2), lrc_right(a, rrow, u0 + 3));
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int u = cb + e * 64 + lane;
        if (u >= a.W) break;
        const int32_t rl = a.left[row + u];
        const uint32_t m = lrc_reason(a, rrow, u, rl);
        cnt += m == SN_LRC_KEPT;
        if (a.out_raw) a.out_raw[row + u] = m ? 0 : rl;
        if (a.mask) a.mask[row + u] = (uint8_t)m;
        if (a.disp && m) a.disp[row + u] = 0.f;
        if (a.right_out) a.right_out[row + u] = lrc_right(a, rrow, u);
      }
    }
  }
  if (a.kept) {
    const uint32_t total = pc_block_sum(cnt, red);
    if (threadIdx.x == 0 && total) atomicAdd(a.kept + k, total);
  }
}

}  // namespace sn
