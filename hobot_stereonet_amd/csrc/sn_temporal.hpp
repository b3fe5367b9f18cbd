// sn_temporal.hpp — temporal filter of int32 disparity streams (sn_temporal_push; the contract is in include/stereonet_hip.h,
// the numpy twin is hobot_stereonet_amd/temporal.py).  All per-pixel arithmetic is integer; the one float operation is the
// multiply for disp.
//
//   k_temporal<VEC, LUMA>  grid (pixel chunks, streams present in the launch), 256 threads.  The host sorts the launch's maps by
//                 stream (TmpArgs::first / map: group g owns map[first[g] .. first[g + 1]), in time order).  A lane owns PX
//                 consecutive pixels (VEC: 4, else 1) of ONE stream and walks that stream's frames with P, Hs and Yp in
//                 registers: the state is read once before the first frame (not at all for a fresh stream: P = Hs = 0 and "no
//                 previous luma" are the host's flag, so a reset needs no memset) and written once after the last, and two
//                 workgroups never touch the same state word.  Pointwise, so out_raw == raw needs no copy.
//                 VEC (W % 4 == 0 and aligned pointers; four pixels never straddle a row): 16-byte loads and stores of the maps
//                 and of P, 4-byte ones of luma, mask, Hs and Yp.  Otherwise one pixel per lane (1242 x 375; NV12 at an odd
//                 offset or pitch).
//                 LUMA = false (luma_delta == 0): no guide is read, Yp is neither read nor written.
//                 Traffic per pixel and frame: raw 4 + luma 1 + out 4 + mask 1 (+ disp 4 where it changes), and 6 (+ 6) bytes
//                 of state per pixel and launch.
//                 counts: sn_streams.hpp's stats_*.  No barrier inside the frame loop.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/stereonet_hip.h"   // SN_TMP_*
#include "sn_streams.hpp"

namespace sn {

struct TmpArgs {
  const int32_t* raw;    // [m][H][W]; may be out_raw
  const uint8_t* luma;   // Y(k, v, u) = luma[k * luma_frame + v * luma_pitch + u] ^ luma_xor; unused without LUMA
  int32_t* out_raw;      // nullable
  float* disp;           // nullable
  uint8_t* mask;         // nullable
  uint32_t* counts;      // nullable: [m][4], zeroed before the launch
  int32_t* P;            // state [streams][H*W]
  uint8_t* Hs;
  uint8_t* Yp;
  size_t luma_frame;
  int luma_pitch;
  uint32_t luma_xor;     // 0 (NV12) or 0x80 (the int8 model input)
  int W, H;
  int alpha, persist, luma_delta;
  long long q;
  float S;
  StreamGroups g;        // the launch's maps, sorted by stream
};

// the contract for one pixel and frame: updates P, Hs, Yp; returns the mask bits and sets *out
template <bool LUMA>
__device__ __forceinline__ uint32_t tmp_step(const TmpArgs& a, bool seen, int32_t raw, uint32_t y, int32_t& P, uint32_t& Hs,
                                             uint32_t& Yp, int32_t* out) {
  const int32_t r = raw > 0 ? raw : 0;
  bool moved = false;
  if (LUMA) {
    const int dy = (int)y - (int)Yp;
    moved = seen && (dy < 0 ? -dy : dy) > a.luma_delta;
  }
  uint32_t bits = 0;
  int32_t o;
  if (r > 0) {
    long long d = (long long)r - (long long)P;
    d = d < 0 ? -d : d;
    if (P > 0 && !moved && d <= a.q) {
      o = (int32_t)(((long long)a.alpha * r + (long long)(256 - a.alpha) * P + 128) >> 8);
      bits = o != r ? (uint32_t)SN_TMP_BLENDED : 0u;
    } else {
      o = r;
      if (P > 0) bits = moved ? (uint32_t)SN_TMP_MOVED : (uint32_t)SN_TMP_JUMP;
    }
    P = o;
  } else {
    bits = SN_TMP_INVALID_IN;
    if (a.persist > 0 && P > 0 && !moved && __popc(Hs) >= a.persist) {
      o = P;
      bits |= SN_TMP_HELD;
    } else {
      o = 0;
      if (P > 0 && moved) {
        bits |= SN_TMP_MOVED;
        P = 0;
      }
    }
  }
  Hs = ((Hs << 1) | (r > 0 ? 1u : 0u)) & 255u;
  if (Hs == 0) P = 0;
  if (LUMA) Yp = y;
  *out = o;
  return bits;
}

// grid (ceil(H*W / (256 * PX)), groups)
template <bool VEC, bool LUMA>
__global__ __launch_bounds__(256) void k_temporal(TmpArgs a) {
  constexpr int PX = VEC ? 4 : 1;
  __shared__ uint32_t cnt[kSlice][4];
  const int g = blockIdx.y, f0 = a.g.first[g], f1 = a.g.first[g + 1];
  const size_t HW = (size_t)a.H * a.W;
  const size_t p0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * PX;
  const bool live = p0 < HW;      // VEC: H*W is a multiple of 4, so the lane's four pixels are all inside or all outside
  if (a.counts) {
    stats_clear(cnt, f1 - f0);
    __syncthreads();
  }
  const size_t sp = (size_t)a.g.stream[g] * HW + p0;
  bool seen = !a.g.fresh[g];
  int32_t P[PX];
  uint32_t Hs[PX], Yp[PX];
#pragma unroll
  for (int e = 0; e < PX; ++e) P[e] = 0, Hs[e] = 0, Yp[e] = 0;
  if (live && seen) {
    if constexpr (VEC) {
      const int4 p = *reinterpret_cast<const int4*>(a.P + sp);
      const uint32_t hs = *reinterpret_cast<const uint32_t*>(a.Hs + sp);
      const uint32_t yp = LUMA ? *reinterpret_cast<const uint32_t*>(a.Yp + sp) : 0u;
      const int32_t pe[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
      for (int e = 0; e < PX; ++e) P[e] = pe[e], Hs[e] = (hs >> (8 * e)) & 255u, Yp[e] = (yp >> (8 * e)) & 255u;
    } else {
      P[0] = a.P[sp];
      Hs[0] = a.Hs[sp];
      if (LUMA) Yp[0] = a.Yp[sp];
    }
  }
  size_t loff = 0;
  if (LUMA) {
    const size_t v = p0 / a.W;
    loff = v * a.luma_pitch + (p0 - v * a.W);
  }
#pragma unroll 1
  for (int f = f0; f < f1; ++f) {
    const int k = a.g.map[f];
    const size_t mp = (size_t)k * HW + p0;
    uint32_t n_valid = 0, n_blend = 0, n_held = 0, n_reset = 0;
    if (live) {
      int32_t r[PX], o[PX];
      uint32_t y[PX], m[PX];
      if constexpr (VEC) {
        const int4 x = *reinterpret_cast<const int4*>(a.raw + mp);
        const int32_t xe[4] = {x.x, x.y, x.z, x.w};
        const uint32_t yy = LUMA ? *reinterpret_cast<const uint32_t*>(a.luma + (size_t)k * a.luma_frame + loff) ^ (a.luma_xor * 0x01010101u) : 0u;
#pragma unroll
        for (int e = 0; e < PX; ++e) r[e] = xe[e], y[e] = (yy >> (8 * e)) & 255u;
      } else {
        r[0] = a.raw[mp];
        y[0] = LUMA ? (uint32_t)(a.luma[(size_t)k * a.luma_frame + loff] ^ a.luma_xor) & 255u : 0u;
      }
#pragma unroll
      for (int e = 0; e < PX; ++e) {
        m[e] = tmp_step<LUMA>(a, seen, r[e], y[e], P[e], Hs[e], Yp[e], &o[e]);
        n_valid += o[e] > 0;
        n_blend += (m[e] & SN_TMP_BLENDED) != 0;
        n_held += (m[e] & SN_TMP_HELD) != 0;
        n_reset += (m[e] & (SN_TMP_MOVED | SN_TMP_JUMP)) != 0;
      }
      if constexpr (VEC) {
        if (a.out_raw) *reinterpret_cast<int4*>(a.out_raw + mp) = make_int4(o[0], o[1], o[2], o[3]);
        if (a.mask) *reinterpret_cast<uint32_t*>(a.mask + mp) = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
      } else {
        if (a.out_raw) a.out_raw[mp] = o[0];
        if (a.mask) a.mask[mp] = (uint8_t)m[0];
      }
      if (a.disp) {
#pragma unroll
        for (int e = 0; e < PX; ++e)
          if (o[e] != (r[e] > 0 ? r[e] : 0)) a.disp[mp + e] = (float)o[e] * a.S;
      }
    }
    seen = true;
    if (a.counts) stats_frame(cnt[f - f0], n_valid | (n_blend << 16), n_held | (n_reset << 16));      // wave-uniform; a wave's sums are at most 256
  }
  if (live && f1 > f0) {
    if constexpr (VEC) {
      *reinterpret_cast<int4*>(a.P + sp) = make_int4(P[0], P[1], P[2], P[3]);
      *reinterpret_cast<uint32_t*>(a.Hs + sp) = Hs[0] | (Hs[1] << 8) | (Hs[2] << 16) | (Hs[3] << 24);
      if (LUMA) *reinterpret_cast<uint32_t*>(a.Yp + sp) = Yp[0] | (Yp[1] << 8) | (Yp[2] << 16) | (Yp[3] << 24);
    } else {
      a.P[sp] = P[0];
      a.Hs[sp] = (uint8_t)Hs[0];
      if (LUMA) a.Yp[sp] = (uint8_t)Yp[0];
    }
  }
  if (a.counts) stats_flush(cnt, a.counts, a.g.map, f0, f1);
}

}  // namespace sn
