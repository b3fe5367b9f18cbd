// sn_confidence.hpp — per-pixel confidence of the disparity map and the mask on it (sn_infer_conf, sn_conf_mask; the contract
// is in include/stereonet_hip.h).  The low-resolution plane conf_low [n][hl][wl] is written by the soft-argmin epilogue
// (softargmin_conf, sn_kernels.hpp); this file brings it to the map's size and applies the threshold.
//
//   k_conf_apply<true>   conf[y][x] = upsample_map(conf_low, hl, wl, y, x, UpScale{1/16, 1}): the device function and the
//                        convention (half-pixel centres, edge clamp) that feed the refinement its disparity, factor 1 on the
//                        values.  The x16 sample positions are multiples of 1/32, so the bilinear weights are exact in fp32.
//   k_conf_apply<false>  reads a full-resolution conf [n][H][W] instead (sn_conf_mask, stateless).
// One thread per output pixel, lanes along x: every load and store of a wave is one contiguous run of a row (the four taps
// of conf_low come from at most two 14 KB planes' worth of lines that stay in the L1 / L2).  The kernel is memory-bound:
// per pixel it reads 4 bytes of raw and writes 4 (conf) + 4 (raw) + 1 (mask) bytes, plus 4 of disp at a rejected pixel.
// kept[k]: a ballot per 64-pixel run, summed per wave, ONE integer atomicAdd per wave (integer, order-free: deterministic).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/stereonet_hip.h"   // SN_CONF_*

namespace sn {

struct ConfArgs {
  const float* conf_in;    // LOW: conf_low [n][hl][wl]; else conf [n][H][W]
  const int32_t* raw;      // [n][H][W]; only read when masking
  float* out_conf;         // nullable [n][H][W] (LOW only)
  int32_t* out_raw;        // nullable; may be `raw`
  float* disp;             // nullable: 0.0f is written at the rejected pixels only
  uint8_t* mask;           // nullable: SN_CONF_* per pixel
  uint32_t* kept;          // nullable: [n], zeroed before the launch
  int hl, wl, H, W;
  float min_conf;
  int masking;             // 0: out_conf only (no threshold given)
};

// grid (workgroups per map, n): every wave walks 64-pixel runs of map blockIdx.y with the grid's stride and ends with its one
// atomic.  The launcher keeps the grid at about 1024 workgroups: atomics that meet on one address are resolved one after the
// other at about 10 ns each (the refinement statistic's measurement: sn_kernels.hpp above refine_stat_commit,
// profiles/r06_stat_atomics.txt), and kept[k] is one word per map.  One wave per 64-pixel run would be 14,400 atomics per
// 1280x720 map, of the order of 0.1 ms by that figure, against the few microseconds the map's bytes take: the number of
// waves, not of pixels, sets the atomics' cost, so a wave walks many runs and commits once.
template <bool LOW>
__global__ __launch_bounds__(256) void k_conf_apply(ConfArgs a) {
  const int k = blockIdx.y, lane = threadIdx.x & 63;
  const int HW = a.H * a.W;
  uint32_t cnt = 0;                  // wave-uniform
  for (int base = blockIdx.x * 256 + (threadIdx.x & ~63); base < HW; base += gridDim.x * 256) {
    const int idx = base + lane;
    uint32_t m = 1;                  // a lane without a pixel counts as rejected
    if (idx < HW) {
      const size_t g = (size_t)k * HW + idx;
      float c;
      if (LOW) {
        const int y = idx / a.W, x = idx - y * a.W;
        c = upsample_map(a.conf_in + (size_t)k * a.hl * a.wl, a.hl, a.wl, y, x, UpScale{1.0f / 16.0f, 1.0f});
        if (a.out_conf) a.out_conf[g] = c;
      } else {
        c = a.conf_in[g];
      }
      if (a.masking) {
        const int32_t r = a.raw[g];
        m = r <= 0 ? SN_CONF_INVALID_IN : (!(c >= a.min_conf) ? SN_CONF_LOW : SN_CONF_KEPT);     // NaN: rejected
        if (a.out_raw) a.out_raw[g] = m ? 0 : r;
        if (a.mask) a.mask[g] = (uint8_t)m;
        if (a.disp && m) a.disp[g] = 0.f;
      }
    }
    if (a.masking && a.kept) cnt += (uint32_t)__popcll(__ballot(m == SN_CONF_KEPT));      // uniform
  }
  if (lane == 0 && cnt) atomicAdd(a.kept + k, cnt);
}

}  // namespace sn
