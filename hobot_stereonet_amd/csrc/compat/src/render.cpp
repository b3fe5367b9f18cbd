// render.cpp — see render.h.  Follows publisher_member_function.py:57-137 of the reference's render node.
#include "render.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace hobot {
namespace stereonet {

namespace {
struct Jet {
  uint8_t t[256 * 3];
  Jet() {
    auto ramp = [](double x, double centre) {
      double v = 1.5 - std::fabs(4.0 * x - centre);
      return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
    };
    for (int i = 0; i < 256; ++i) {
      const double x = i / 255.0;
      t[3 * i + 0] = (uint8_t)std::nearbyint(ramp(x, 1.0) * 255.0);   // B
      t[3 * i + 1] = (uint8_t)std::nearbyint(ramp(x, 2.0) * 255.0);   // G
      t[3 * i + 2] = (uint8_t)std::nearbyint(ramp(x, 3.0) * 255.0);   // R
    }
  }
};
}  // namespace

const uint8_t* JetLutBGR() {
  static const Jet jet;
  return jet.t;
}

uint8_t ConvertScaleAbs(double v, double alpha) {
  const double a = std::fabs(v * alpha);
  if (std::isnan(a)) return 0;
  const double r = std::nearbyint(a);      // round-half-even in the default rounding mode, as cvRound
  return r >= 255.0 ? 255 : (uint8_t)r;
}

bool RenderDepth(const uint8_t* payload, size_t len, int w, int h, const RenderConstants& k, double* disp, double* depth,
                 uint8_t* color_bgr, size_t* jpeg_off) {
  const size_t n = (size_t)w * h;
  if (!payload || w <= 0 || h <= 0 || len < n * 4) return false;
  if (jpeg_off) *jpeg_off = n * 4;
  const uint8_t* lut = JetLutBGR();
  for (size_t i = 0; i < n; ++i) {
    uint32_t raw;
    memcpy(&raw, payload + 4 * i, 4);                          // :65-66 np.uint32 view
    const double d = (double)raw * k.scale * 16.0 * 12.0;      // :73-75
    const double z = k.focal * k.baseline / d / 1000.0;        // :81 (zero disparity -> inf, kept)
    if (disp) disp[i] = d;
    if (depth) depth[i] = z;
    if (color_bgr) memcpy(color_bgr + 3 * i, lut + 3 * ConvertScaleAbs(z, k.alpha), 3);   // :82
  }
  return true;
}

void StackJoint(const uint8_t* left_rgb, const uint8_t* color_bgr, int w, int h, std::vector<uint8_t>& joint_rgb) {
  const size_t n = (size_t)w * h * 3;
  joint_rgb.resize(2 * n);
  memcpy(joint_rgb.data(), left_rgb, n);
  memcpy(joint_rgb.data() + n, color_bgr, n);                  // BGR bytes published as if they were RGB (:108-137)
}


bool RenderTables(const RenderParams& p, uint8_t* rgb, uint8_t* ycc) {
  if (p.colormap != kCmapJet && p.colormap != kCmapGrey) return false;
  const uint8_t* jet = JetLutBGR();
  for (int i = 0; i < 257; ++i) {
    uint8_t c[3] = {0, 0, 0};      // entry 256 is black
    if (i < 256) {
      for (int e = 0; e < 3; ++e) c[e] = p.colormap == kCmapJet ? jet[3 * i + e] : (uint8_t)i;
      if (p.true_colours) std::swap(c[0], c[2]);      // (B, G, R) -> (R, G, B); otherwise B, G, R stand where R, G, B belong
    }
    const int R = c[0], G = c[1], B = c[2];
    if (rgb) memcpy(rgb + 3 * i, c, 3);
    if (ycc) {
      ycc[3 * i] = (uint8_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
      ycc[3 * i + 1] = (uint8_t)((-11059 * R - 21709 * G + 32768 * B + 8388608 + 32767) >> 16);
      ycc[3 * i + 2] = (uint8_t)((32768 * R - 27439 * G - 5329 * B + 8388608 + 32767) >> 16);
    }
  }
  return true;
}

namespace {
int Clamp255(int x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }
}  // namespace

bool RenderCanvas(const int32_t* raw, const uint8_t* left_nv12, int left_pitch, int w, int h, const RenderParams& p, int format,
                  uint8_t* out, int out_pitch) {
  const bool stack = p.layout == kRenderStack, nv12 = format == kRenderNv12;
  uint8_t rgb[257 * 3], ycc[257 * 3];
  if (!raw || !out || w <= 0 || h <= 0 || (!stack && p.layout != kRenderDepth) || (!nv12 && format != kRenderRgb8) ||
      !RenderTables(p, rgb, ycc) || (stack && (!left_nv12 || left_pitch < w || (left_pitch & 1))) || (nv12 && ((w | h) & 1)) ||
      out_pitch < (nv12 ? w : 3 * w))
    return false;
  const double scale = p.scale == 0 ? 0.00000260443857769133 : p.scale, focal = p.focal_px == 0 ? 527.1931762695312 : p.focal_px;
  const double baseline = p.baseline_mm == 0 ? 119.89382172 : p.baseline_mm, alpha = p.alpha == 0 ? 9.0 : p.alpha;
  std::vector<uint16_t> idx((size_t)w * h);
  for (size_t i = 0; i < idx.size(); ++i) {
    uint32_t r;
    memcpy(&r, raw + i, 4);
    const double d = (double)r * scale * 16.0 * 12.0;      // RenderDepth's order of operations
    const double z = focal * baseline / d / 1000.0;
    idx[i] = r == 0 && p.invalid_black ? 256 : ConvertScaleAbs(z, alpha);
  }
  const int hc = stack ? 2 * h : h, top = stack ? h : 0;
  if (!nv12) {
    for (int v = 0; stack && v < h; ++v)
      for (int u = 0; u < w; ++u) {      // sn_pointcloud_from_raw's integer BT.601, true NV12 chroma siting
        const int y = left_nv12[(size_t)v * left_pitch + u];
        const uint8_t* uv = left_nv12 + (size_t)(h + (v >> 1)) * left_pitch + (u & ~1);
        const int uc = (int)uv[0] - 128, vc = (int)uv[1] - 128;
        uint8_t* o = out + (size_t)v * out_pitch + 3 * u;
        o[0] = (uint8_t)Clamp255(y + ((91881 * vc + 32768) >> 16));
        o[1] = (uint8_t)Clamp255(y + ((-22554 * uc - 46802 * vc + 32768) >> 16));
        o[2] = (uint8_t)Clamp255(y + ((116130 * uc + 32768) >> 16));
      }
    for (int v = 0; v < h; ++v)
      for (int u = 0; u < w; ++u) memcpy(out + (size_t)(top + v) * out_pitch + 3 * u, rgb + 3 * idx[(size_t)v * w + u], 3);
    return true;
  }
  for (int v = 0; stack && v < h + h / 2; ++v)      // the left eye's luma rows, and its chroma rows behind the canvas's luma
    memcpy(out + (size_t)(v < h ? v : hc + v - h) * out_pitch, left_nv12 + (size_t)v * left_pitch, w);
  for (int v = 0; v < h; ++v)
    for (int u = 0; u < w; ++u) out[(size_t)(top + v) * out_pitch + u] = ycc[3 * idx[(size_t)v * w + u]];
  for (int v = 0; v < h; v += 2)
    for (int u = 0; u < w; u += 2)
      for (int e = 1; e < 3; ++e) {
        const size_t i = (size_t)v * w + u;
        const int sum = ycc[3 * idx[i] + e] + ycc[3 * idx[i + 1] + e] + ycc[3 * idx[i + w] + e] + ycc[3 * idx[i + w + 1] + e];
        out[(size_t)(hc + (top + v) / 2) * out_pitch + u + e - 1] = (uint8_t)((sum + 2) >> 2);
      }
  return true;
}

}  // namespace stereonet
}  // namespace hobot
