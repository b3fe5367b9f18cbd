// sn_smooth.hpp — guided weighted-median smoothing of int32 disparity maps (sn_smooth_raw; the contract is in
// include/stereonet_hip.h, the numpy twin is hobot_stereonet_amd/smooth.py).  All per-pixel arithmetic is integer.
//
//   k_smooth<R, WEIGHTED>  one workgroup per 64 x 16 tile, grid (tiles, maps).  The tile and its halo of R pixels are staged in
//                 LDS once — max(raw, 0) as int32 (0 outside the image: such a pixel never takes part), the luma as bytes, the
//                 256-entry weight table as 16-bit words — so every window read is an LDS read and every global byte is read
//                 once per tile (the halo: (64 + 2R)(16 + 2R) / 1024 = 1.2 .. 1.5 times per map).  A wave owns four tile rows,
//                 lane = column, one pixel per lane at a time: the window's K = (2R+1)^2 values and weights sit in 2K registers
//                 (K for the unweighted form), a pixel that does not take part as the pair (INT32_MAX, 0).  The lower weighted
//                 median is found by rank counting: every window pixel in turn is the candidate c (read again from LDS, so the
//                 outer loop indexes no register), S(c) = the sum of w_j over v_j <= c is K compare-select-add steps over the
//                 registers, fully unrolled, and the answer is the smallest c with 2 S(c) >= Wt.  A non-participant is a
//                 harmless candidate: its INT32_MAX always qualifies and never beats a participant, the largest of which
//                 qualifies too.  K^2 steps per pixel: 81, 625, 2401 for R = 1, 2, 3.
//                 WEIGHTED = false (sigma_luma == 0): no luma, no table, the weights are the participation bits.
//                 First-touch traffic: raw 4 (+ halo) + luma 1 (+ halo) + out 4 + mask 1 + disp 4 bytes per pixel.
//                 counts: per-thread integers, one atomicAdd per workgroup and counter.  No other atomics, no floating point
//                 but the one multiply for disp.
// The kernel reads a halo that another workgroup may own, so it never works in place: for out_raw == raw the entry point hands
// it a copy of the slice (the scratch).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sn_pointcloud.hpp"   // pc_block_sum
#include "../../include/stereonet_hip.h"   // SN_SMOOTH_*

namespace sn {

constexpr int kSmTW = 64, kSmTH = 16;
constexpr int kSmSlice = 8;      // maps per pass over the scratch (4 bytes per pixel and map, in-place calls only)

struct SmArgs {
  const int32_t* raw;    // [n][H][W]; never the same memory as out_raw
  const uint8_t* luma;   // Y(k, v, u) = luma[k * luma_frame + v * luma_pitch + u] ^ luma_xor; unused when unweighted
  int32_t* out_raw;      // nullable
  float* disp;           // nullable
  uint8_t* mask;         // nullable
  uint32_t* counts;      // nullable: [n][3], zeroed before the launch
  size_t luma_frame;
  int luma_pitch;
  uint32_t luma_xor;     // 0 (NV12) or 0x80 (the int8 model input)
  int W, H, tiles_x;
  int min_valid;
  float S;
  uint16_t table[256];   // T[|luma difference|], 0..256
};

// grid (tiles_x * tiles_y, maps)
template <int R, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_smooth(SmArgs a) {
  constexpr int D = 2 * R + 1, K = D * D, PW = kSmTW + 2 * R, PH = kSmTH + 2 * R;
  constexpr int32_t kNone = 0x7fffffff;
  __shared__ int32_t sraw[PH * PW];
  __shared__ uint8_t sluma[WEIGHTED ? PH * PW : 4];
  __shared__ uint16_t stab[256];
  __shared__ uint32_t red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int x0 = tx * kSmTW, y0 = ty * kSmTH;
  const size_t map = (size_t)blockIdx.y * a.H * a.W;
  const int32_t* raw = a.raw + map;
  const uint8_t* luma = WEIGHTED ? a.luma + (size_t)blockIdx.y * a.luma_frame : nullptr;
  for (int i = threadIdx.x; i < PH * PW; i += 256) {
    const int ly = i / PW, lx = i - ly * PW;
    const int y = y0 - R + ly, x = x0 - R + lx;
    const bool in = x >= 0 && x < a.W && y >= 0 && y < a.H;
    const int32_t r = in ? raw[(size_t)y * a.W + x] : 0;
    sraw[i] = r > 0 ? r : 0;
    if (WEIGHTED) sluma[i] = in ? (uint8_t)(luma[(size_t)y * a.luma_pitch + x] ^ a.luma_xor) : (uint8_t)0;
  }
  if (WEIGHTED) stab[threadIdx.x] = a.table[threadIdx.x];
  __syncthreads();
  uint32_t n_valid = 0, n_smoothed = 0, n_filled = 0;
  const int x = x0 + lane;
#pragma unroll 1
  for (int e = 0; e < 4; ++e) {
    const int r = wave * 4 + e, y = y0 + r;
    if (y >= a.H) break;                                 // wave-uniform
    const int32_t* win = sraw + r * PW + lane;           // the window's top-left pixel
    const uint8_t* lwin = sluma + r * PW + lane;
    const int32_t centre = win[R * PW + R];
    const int yc = WEIGHTED ? lwin[R * PW + R] : 0;
    int32_t v[K];
    int w[WEIGHTED ? K : 1];
    int wt = 0, measured = 0;
#pragma unroll
    for (int dy = 0; dy < D; ++dy)
#pragma unroll
      for (int dx = 0; dx < D; ++dx) {
        const int32_t q = win[dy * PW + dx];
        int wq = q > 0;
        measured += wq;
        if (WEIGHTED) {
          const int dl = (int)lwin[dy * PW + dx] - yc;
          const int t = stab[dl < 0 ? -dl : dl];      // read unconditionally: no divergence
          wq = q > 0 ? t : 0;
          w[dy * D + dx] = wq;
        }
        v[dy * D + dx] = wq > 0 ? q : kNone;
        wt += wq;
      }
    int32_t m = kNone;
#pragma unroll 1
    for (int dy = 0; dy < D; ++dy) {
#pragma unroll
      for (int dx = 0; dx < D; ++dx) {
        const int32_t q = win[dy * PW + dx];
        bool part = q > 0;
        if (WEIGHTED) {
          const int dl = (int)lwin[dy * PW + dx] - yc;
          const int t = stab[dl < 0 ? -dl : dl];
          part = q > 0 && t != 0;
        }
        const int32_t c = part ? q : kNone;
        int s = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) s += v[j] <= c ? (WEIGHTED ? w[j] : 1) : 0;
        if (2 * s >= wt && c < m) m = c;
      }
    }
    int32_t res;
    if (centre > 0) res = m;                             // the centre takes part with T[0] > 0
    else res = (a.min_valid > 0 && measured >= a.min_valid && wt > 0) ? m : 0;
    if (x >= a.W) continue;
    const uint32_t bits = (centre > 0 ? 0u : (uint32_t)SN_SMOOTH_INVALID_IN) | (res != centre ? (uint32_t)SN_SMOOTH_CHANGED : 0u);
    n_valid += res > 0;
    n_smoothed += centre > 0 && res != centre;
    n_filled += centre <= 0 && res != centre;
    const size_t p = map + (size_t)y * a.W + x;
    if (a.out_raw) a.out_raw[p] = res;
    if (a.mask) a.mask[p] = (uint8_t)bits;
    if (a.disp && (bits & SN_SMOOTH_CHANGED)) a.disp[p] = res > 0 ? (float)res * a.S : 0.f;
  }
  if (a.counts) {
    const uint32_t t0 = pc_block_sum(n_valid, red), t1 = pc_block_sum(n_smoothed, red), t2 = pc_block_sum(n_filled, red);
    if (threadIdx.x == 0) {
      if (t0) atomicAdd(a.counts + blockIdx.y * 3 + 0, t0);
      if (t1) atomicAdd(a.counts + blockIdx.y * 3 + 1, t1);
      if (t2) atomicAdd(a.counts + blockIdx.y * 3 + 2, t2);
    }
  }
}

}  // namespace sn
