// sn_rectify.hpp — stereo rectification of raw NV12 pairs (sn_rectify_*; the contract, Stage A and Stage B, is in
// include/stereonet_hip.h, the numpy twin is hobot_stereonet_amd/rectify.py).
//
//   rectify_build_map  Stage A on the host, in double, under `#pragma clang fp contract(off)`: the order of operations is the
//                 contract, and no build flag may fuse a multiply into an add.
//   k_rectify     Stage B.  grid (chunks of 256 items, eye), 256 threads.  An item is 4 consecutive destination bytes of one eye
//                 in the side-by-side frame: 4 luma pixels, or 2 UV pairs of a chroma row (W % 4 == 0, so an item never
//                 straddles a row or an eye).  A lane loads the item's map entries once (two 16-byte loads; the chroma
//                 section reads the luma map at even rows and columns), turns them into 16 byte offsets into an eye's source
//                 image, 16 weights and 4 constants — all of them the same for every frame — and then walks the call's n
//                 frames with those in registers, as k_temporal walks a stream's frames: per frame 16 byte loads, issued
//                 before the first blend, and one 32-bit store.  A tap outside the source plane (and every tap of a
//                 sentinel) keeps weight 0 and offset 0 and adds weight * B to the item's constant instead, so the frame loop
//                 has no branch.  Source pointers need no alignment: the taps are byte loads, and neighbouring lanes' taps
//                 are neighbours in the source, so a wave's loads fall into a few cache lines.  No LDS, no atomics.
//                 Traffic per call: the map once (16 bytes per luma pixel and eye, a quarter of it again for the chroma
//                 section), per frame the source once and the destination once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/stereonet_hip.h"

namespace sn {

constexpr int32_t kRectSentinel = INT32_MIN;

struct RectArgs {
  const uint8_t* src[2];   // pair 0's left and right eye; pair k at + k * src_frame
  const int32_t* map;      // [2][H][W][2]
  uint8_t* out;            // [n] side-by-side frames of pitch 2W
  size_t src_frame;
  int src_pitch, sw, sh;
  int W, H, n;
};

inline bool rect_eye_ok(const sn_eye_calib& e) {
  bool ok = std::isfinite(e.fx) && std::isfinite(e.fy) && std::isfinite(e.cx) && std::isfinite(e.cy) && e.fx > 0 && e.fy > 0;
  for (double v : e.d) ok = ok && std::isfinite(v);
  for (double v : e.R) ok = ok && std::isfinite(v);
  return ok;
}

inline bool rect_calib_ok(const sn_stereo_calib* c) {
  return c && c->src_w >= 2 && c->src_w <= 8192 && c->src_h >= 2 && c->src_h <= 8192 && !(c->src_w & 1) && !(c->src_h & 1) &&
         rect_eye_ok(c->left) && rect_eye_ok(c->right) && std::isfinite(c->pfx) && std::isfinite(c->pfy) &&
         std::isfinite(c->pcx) && std::isfinite(c->pcy) && std::isfinite(c->baseline_mm) && c->pfx > 0 && c->pfy > 0 &&
         c->baseline_mm > 0;
}

// Stage A for one eye; returns the number of entries that are not the sentinel
inline uint32_t rectify_build_map(const sn_stereo_calib& c, int eye, int w, int h, int32_t* map_xy) {
#pragma clang fp contract(off)
  const sn_eye_calib& e = eye ? c.right : c.left;
  const double* R = e.R;
  const double k1 = e.d[0], k2 = e.d[1], p1 = e.d[2], p2 = e.d[3], k3 = e.d[4];
  const double sw = (double)c.src_w, sh = (double)c.src_h;
  uint32_t valid = 0;
  for (int v = 0; v < h; ++v) {
    const double y = ((double)v - c.pcy) / c.pfy;
    for (int u = 0; u < w; ++u) {
      int32_t* m = map_xy + ((size_t)v * w + u) * 2;
      m[0] = m[1] = kRectSentinel;
      const double x = ((double)u - c.pcx) / c.pfx;
      const double X = R[0] * x + R[3] * y + R[6];
      const double Y = R[1] * x + R[4] * y + R[7];
      const double Wc = R[2] * x + R[5] * y + R[8];
      if (!(Wc > 0)) continue;
      const double a = X / Wc, b = Y / Wc, a2 = a * a, b2 = b * b, r2 = a2 + b2, ab2 = 2.0 * (a * b);
      const double rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
      const double xd = a * rad + (p1 * ab2 + p2 * (r2 + 2.0 * a2));
      const double yd = b * rad + (p1 * (r2 + 2.0 * b2) + p2 * ab2);
      const double us = e.fx * xd + e.cx, vs = e.fy * yd + e.cy;
      if (!(us > -1 && us < sw && vs > -1 && vs < sh)) continue;
      m[0] = (int32_t)std::floor(us * 256.0 + 0.5);
      m[1] = (int32_t)std::floor(vs * 256.0 + 0.5);
      ++valid;
    }
  }
  return valid;
}

// one map entry -> the four taps of one output byte: offsets (relative to the plane's first byte, `step` bytes per sample),
// weights and the constant 32768 + the border's share.  (mx, my) is a Q8 coordinate on a pw x ph plane.
__device__ __forceinline__ void rect_taps(int32_t mx, int32_t my, bool sentinel, int pw, int ph, int pitch, int step, uint32_t B,
                                          uint32_t off[4], uint32_t wt[4], uint32_t* base) {
  const int x0 = mx >> 8, y0 = my >> 8;
  const uint32_t fx = (uint32_t)mx & 255u, fy = (uint32_t)my & 255u;
  const uint32_t w4[4] = {(256u - fx) * (256u - fy), fx * (256u - fy), (256u - fx) * fy, fx * fy};
  uint32_t c = 32768u;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int x = x0 + (t & 1), y = y0 + (t >> 1);
    const bool in = !sentinel && (unsigned)x < (unsigned)pw && (unsigned)y < (unsigned)ph;
    off[t] = in ? (uint32_t)y * (uint32_t)pitch + (uint32_t)x * (uint32_t)step : 0u;
    wt[t] = in ? w4[t] : 0u;
    c += in ? 0u : w4[t] * B;
  }
  *base = sentinel ? (B << 16) + 32768u : c;
}

// grid (ceil((H + H/2) * (W/4) / 256), 2)
__global__ __launch_bounds__(256) void k_rectify(RectArgs a) {
  const int quads = a.W >> 2;
  const int item = blockIdx.x * 256 + threadIdx.x;      // < 2^31: (H + H/2) * W/4 of a model image
  if (item >= (a.H + (a.H >> 1)) * quads) return;
  const int eye = blockIdx.y;
  const int row = item / quads, q = item - row * quads;
  const bool chroma = row >= a.H;
  // the item's map entries: luma (row, 4q .. 4q+3); chroma row ci = row - H: (2ci, 4q) and (2ci, 4q + 2)
  const int mv = chroma ? 2 * (row - a.H) : row;
  const int4* mp = reinterpret_cast<const int4*>(a.map + (((size_t)eye * a.H + mv) * a.W + 4 * q) * 2);
  const int4 m01 = mp[0], m23 = mp[1];
  uint32_t off[4][4], wt[4][4], base[4];
  if (!chroma) {
    const int32_t mx[4] = {m01.x, m01.z, m23.x, m23.z}, my[4] = {m01.y, m01.w, m23.y, m23.w};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      rect_taps(mx[e], my[e], mx[e] == kRectSentinel && my[e] == kRectSentinel, a.sw, a.sh, a.src_pitch, 1, 0u, off[e], wt[e], &base[e]);
  } else {
    const int32_t mx[2] = {m01.x, m23.x}, my[2] = {m01.y, m23.y};
    const uint32_t plane = (uint32_t)a.sh * (uint32_t)a.src_pitch;      // the chroma rows follow the sh luma rows
#pragma unroll
    for (int e = 0; e < 4; ++e) {      // bytes U0 V0 U1 V1: pair e >> 1, channel e & 1
      const int p = e >> 1;
      const bool sentinel = mx[p] == kRectSentinel && my[p] == kRectSentinel;
      rect_taps(mx[p] >> 1, my[p] >> 1, sentinel, a.sw >> 1, a.sh >> 1, a.src_pitch, 2, 128u, off[e], wt[e], &base[e]);
#pragma unroll
      for (int t = 0; t < 4; ++t) off[e][t] = wt[e][t] ? off[e][t] + plane + (e & 1) : 0u;
    }
  }
  const uint8_t* src = a.src[eye];
  uint8_t* dst = a.out + (size_t)row * (2 * a.W) + (size_t)eye * a.W + 4 * q;
  const size_t out_frame = (size_t)3 * a.W * a.H;
#pragma unroll 1
  for (int k = 0; k < a.n; ++k) {
    uint32_t p[4][4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < 4; ++t) p[e][t] = src[off[e][t]];
    uint32_t word = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t s = base[e] + wt[e][0] * p[e][0] + wt[e][1] * p[e][1] + wt[e][2] * p[e][2] + wt[e][3] * p[e][3];
      word |= (s >> 16) << (8 * e);
    }
    *reinterpret_cast<uint32_t*>(dst) = word;
    src += a.src_frame;
    dst += out_frame;
  }
}

}  // namespace sn
