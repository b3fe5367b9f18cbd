// sn_render.hpp — the depth view of the reference's render node on the GPU (sn_render / sn_render_jpeg; the contract is in
// include/stereonet_hip.h, the numpy twin is hobot_stereonet_amd/render.py, the host C++ twin compat/src/render.cpp).
//
//   render_tables  the two 257-entry tables (canvas bytes and their YCbCr) on the host: a pure function.
//   k_render<NV12> grid (chunks of 256 items, frame), 256 threads.  An item is four columns of two rows of the colour half.  A
//                 lane reads its eight map words (two 16-byte loads where W % 4 == 0 and raw is 16-byte aligned, scalar loads
//                 otherwise), turns each into a colour index in IEEE double under `#pragma clang fp contract(off)` — the order
//                 of operations is the contract — and looks the indices up in the 257-entry table, which the workgroup holds in
//                 LDS as one word per entry (three bytes packed).  RGB8: three dwords per row.  NV12: one luma word per row and
//                 one chroma word (two UV pairs, each the rounded mean of its 2x2 block's table chroma).  The same lane handles
//                 the same 4x2 block of the left eye in the same launch: a copy of two luma words and one chroma word (NV12) or
//                 the point cloud's integer conversion (RGB8: the two rows share their chroma row).  Word accesses where the
//                 base, the pitch and the frame stride are multiples of 4 and the item is whole, byte accesses otherwise (an
//                 odd address, a padded pitch, the last item of a row with W % 4 != 0).  Bytes beyond W (3W) in a row are never
//                 written.  No atomics.  Traffic per frame: the map once (4 bytes a pixel), the left eye once (1.5), the canvas
//                 once (3 or 6 bytes a pixel of the model).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/stereonet_hip.h"

namespace sn {

constexpr int kRenderEntries = 257;      // 0..255: the colour map; 256: "no measurement"

struct RenderArgs {
  const int32_t* raw;      // [n][H][W]
  const uint8_t* left;     // frame k at + k * left_frame (nullptr: SN_RENDER_DEPTH)
  uint8_t* out;            // frame k at + k * out_frame
  size_t left_frame, out_frame;
  double scale, fB, alpha;
  int W, H, left_pitch, out_pitch;
  int stack, invalid_black;
  int vec_raw, word_left, word_out;      // the accesses that may be 16 / 4 bytes wide
  uint32_t tab[kRenderEntries];          // byte0 | byte1 << 8 | byte2 << 16: canvas (R, G, B) or (Y, Cb, Cr)
};

// COLORMAP_JET entry i as (B, G, R): the closed form of compat/src/render.cpp (JetLutBGR) and render.jet_lut()
inline void render_jet_bgr(int i, uint8_t bgr[3]) {
#pragma clang fp contract(off)
  const double x = i / 255.0;
  for (int c = 0; c < 3; ++c) {
    double v = 1.5 - std::fabs(4.0 * x - (double)(c + 1));
    v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
    bgr[c] = (uint8_t)std::nearbyint(v * 255.0);
  }
}

inline bool render_tables(const sn_render_params* p, uint8_t* rgb, uint8_t* ycc) {
  if (!p || (p->colormap != SN_CMAP_JET && p->colormap != SN_CMAP_GREY)) return false;
  for (int i = 0; i < kRenderEntries; ++i) {
    uint8_t c[3] = {0, 0, 0};      // entry 256 is black
    if (i < 256) {
      if (p->colormap == SN_CMAP_JET) render_jet_bgr(i, c);
      else c[0] = c[1] = c[2] = (uint8_t)i;
      if (p->true_colours) {      // (B, G, R) -> (R, G, B); otherwise the table's B, G, R are stored as if they were R, G, B
        const uint8_t t = c[0];
        c[0] = c[2], c[2] = t;
      }
    }
    const int R = c[0], G = c[1], B = c[2];
    if (rgb) rgb[3 * i] = c[0], rgb[3 * i + 1] = c[1], rgb[3 * i + 2] = c[2];
    if (ycc) {
      ycc[3 * i] = (uint8_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
      ycc[3 * i + 1] = (uint8_t)((-11059 * R - 21709 * G + 32768 * B + 8388608 + 32767) >> 16);
      ycc[3 * i + 2] = (uint8_t)((32768 * R - 27439 * G - 5329 * B + 8388608 + 32767) >> 16);
    }
  }
  return true;
}

// the colour index of one map word (viewed as uint32, as the reference does); 256 for "no measurement"
__device__ __forceinline__ uint32_t render_index(uint32_t raw, const RenderArgs& a) {
#pragma clang fp contract(off)
  if (raw == 0u && a.invalid_black) return 256u;
  const double d = (double)raw * a.scale * 16.0 * 12.0;
  const double z = a.fB / d / 1000.0;      // raw == 0 -> +inf
  const double v = fabs(z * a.alpha);
  if (v != v) return 0u;
  const double r = rint(v);                // ties to even
  return r >= 255.0 ? 255u : (uint32_t)(int)r;
}

// nb bytes (1..4) at p, little-endian in a word
__device__ __forceinline__ uint32_t render_load(const uint8_t* p, bool word, int nb) {
  if (word) return *reinterpret_cast<const uint32_t*>(p);
  uint32_t v = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e < nb) v |= (uint32_t)p[e] << (8 * e);
  return v;
}

__device__ __forceinline__ void render_store(uint8_t* p, uint32_t v, bool word, int nb) {
  if (word) {
    *reinterpret_cast<uint32_t*>(p) = v;
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e < nb) p[e] = (uint8_t)(v >> (8 * e));
}

// four pixels' three bytes c[e] = b0 | b1 << 8 | b2 << 16 -> the row's 3 * nc bytes at p
__device__ __forceinline__ void render_store_rgb(uint8_t* p, const uint32_t (&c)[4], bool word, int nc) {
  const uint32_t w[3] = {c[0] | (c[1] << 24), (c[1] >> 8) | (c[2] << 16), (c[2] >> 16) | (c[3] << 8)};
  if (word) {
#pragma unroll
    for (int e = 0; e < 3; ++e) reinterpret_cast<uint32_t*>(p)[e] = w[e];
    return;
  }
#pragma unroll
  for (int e = 0; e < 12; ++e)
    if (e < 3 * nc) p[e] = (uint8_t)(w[e >> 2] >> (8 * (e & 3)));
}

__device__ __forceinline__ uint32_t render_clamp255(int x) { return (uint32_t)(x < 0 ? 0 : (x > 255 ? 255 : x)); }

// grid (ceil(ceil(W / 4) * ceil(H / 2) / 256), n)
template <bool NV12>
__global__ __launch_bounds__(256) void k_render(RenderArgs a) {
  __shared__ uint32_t tab[kRenderEntries];
  for (int i = threadIdx.x; i < kRenderEntries; i += 256) tab[i] = a.tab[i];
  __syncthreads();
  const int quads = (a.W + 3) >> 2, pairs = (a.H + 1) >> 1;
  const int item = blockIdx.x * 256 + threadIdx.x;      // < 2^31: a quarter of a model image's pixels at most
  if (item >= quads * pairs) return;
  const int r = item / quads, q = item - r * quads;
  const int x0 = 4 * q, y0 = 2 * r;
  const int nc = min(4, a.W - x0), nr = min(2, a.H - y0);      // NV12: W and H are even, so nc is 2 or 4 and nr is 2
  const bool whole = nc == 4;
  const size_t k = blockIdx.y;
  const int Hc = a.stack ? 2 * a.H : a.H, top = a.stack ? a.H : 0;      // the canvas rows, the colour half's first row
  uint8_t* out = a.out + k * a.out_frame;

  // ---- the colour half ----
  const int32_t* raw = a.raw + (k * a.H + y0) * a.W + x0;
  uint32_t c[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (j < nr) {
      if (a.vec_raw) {
        const int4 v = *reinterpret_cast<const int4*>(raw + (size_t)j * a.W);
        w[0] = (uint32_t)v.x, w[1] = (uint32_t)v.y, w[2] = (uint32_t)v.z, w[3] = (uint32_t)v.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < nc) w[e] = (uint32_t)raw[(size_t)j * a.W + e];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) c[j][e] = tab[render_index(w[e], a)];      // beyond nc / nr: looked up, never stored
  }
  if (NV12) {
    uint32_t uv = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint32_t y = (c[j][0] & 255u) | ((c[j][1] & 255u) << 8) | ((c[j][2] & 255u) << 16) | ((c[j][3] & 255u) << 24);
      render_store(out + (size_t)(top + y0 + j) * a.out_pitch + x0, y, a.word_out && whole, nc);
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      uint32_t cb = 2u, cr = 2u;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 2; ++e) cb += (c[j][2 * p + e] >> 8) & 255u, cr += (c[j][2 * p + e] >> 16) & 255u;
      uv |= ((cb >> 2) | ((cr >> 2) << 8)) << (16 * p);
    }
    render_store(out + (size_t)(Hc + (top >> 1) + r) * a.out_pitch + x0, uv, a.word_out && whole, nc);
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (j < nr) render_store_rgb(out + (size_t)(top + y0 + j) * a.out_pitch + 3 * x0, c[j], a.word_out && whole, nc);
  }
  if (!a.stack) return;

  // ---- the left eye: the same block; its chroma row r serves both luma rows ----
  const uint8_t* left = a.left + k * a.left_frame;
  const int ncb = 2 * ((nc + 1) >> 1);      // chroma bytes of the block: whole UV pairs
  const uint32_t uv = render_load(left + (size_t)(a.H + r) * a.left_pitch + x0, a.word_left && whole, ncb);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (j >= nr) break;
    const uint32_t y4 = render_load(left + (size_t)(y0 + j) * a.left_pitch + x0, a.word_left && whole, nc);
    if (NV12) {
      render_store(out + (size_t)(y0 + j) * a.out_pitch + x0, y4, a.word_out && whole, nc);
    } else {
      uint32_t px[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {      // sn_pointcloud_from_raw's integer BT.601, true NV12 chroma siting
        const int y = (int)((y4 >> (8 * e)) & 255u);
        const int uc = (int)((uv >> (16 * (e >> 1))) & 255u) - 128, vc = (int)((uv >> (16 * (e >> 1) + 8)) & 255u) - 128;
        px[e] = render_clamp255(y + ((91881 * vc + 32768) >> 16)) |
                (render_clamp255(y + ((-22554 * uc - 46802 * vc + 32768) >> 16)) << 8) |
                (render_clamp255(y + ((116130 * uc + 32768) >> 16)) << 16);
      }
      render_store_rgb(out + (size_t)(y0 + j) * a.out_pitch + 3 * x0, px, a.word_out && whole, nc);
    }
  }
  if (NV12) render_store(out + (size_t)(Hc + r) * a.out_pitch + x0, uv, a.word_out && whole, nc);
}

}  // namespace sn
