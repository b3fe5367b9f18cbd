// sn_weights.hpp — the .snw weight file (SnwHeader, BlobWalker, param_count) and every routine that packs a layer's
// weights into the form its kernel reads and uploads it (upload_*), including the sum-preserving fp16 rounding of the
// tower kernels.  Host code only.  Part of the single translation unit stereonet_hip.hip.
#pragma once

namespace {

// ---- weight file (hobot_stereonet_amd/weights.py documents the layout) -------------------------
struct SnwHeader {
  char magic[4];
  uint32_t version, width, height, dmax, channels, n_down, n_fres, n_agg, n_rres;
  uint32_t dil[6];
  uint64_t n_params, reserved;
};
static_assert(sizeof(SnwHeader) == 80, "SNW1 header is 80 bytes");

struct HostLayer {
  const float* w;
  const float* b;
  int cout, cin, taps;
};

// Walks the canonical tensor order (spec.layers()).
struct BlobWalker {
  const float* base;
  size_t off = 0;
  HostLayer next(int cout, int cin, int taps) {
    HostLayer l{base + off, nullptr, cout, cin, taps};
    off += (size_t)cout * cin * taps;
    l.b = base + off;
    off += cout;
    return l;
  }
};

size_t tower_param_count() {
  return (size_t)kC * 4 * 9 + kC + (size_t)2 * kNRefRes * (kC * kC * 9 + kC) + kC * 9 + 1;
}

size_t param_count(int levels = 1) {
  size_t n = (size_t)(levels - 1) * tower_param_count();
  for (int i = 0; i < kNDown; ++i) n += (size_t)kC * (i == 0 ? 3 : kC) * 25 + kC;
  n += (size_t)(2 * kNFeatRes + 1) * (kC * kC * 9 + kC);
  n += (size_t)kNAgg * (kC * kC * 27 + kC) + kC * 27 + 1;
  n += (size_t)kC * 4 * 9 + kC + (size_t)2 * kNRefRes * (kC * kC * 9 + kC) + kC * 9 + 1;
  return n;
}

// fp32 values / packed fp16 fragments (eight per uint4 slot) to a fresh device buffer
int to_device(sn_handle* h, const float* src, size_t count, float** dst) {
  HIP_TRY(h, dalloc(dst, count));
  HIP_TRY(h, hipMemcpy(*dst, src, count * sizeof(float), hipMemcpyHostToDevice));
  return SN_OK;
}
int to_device(sn_handle* h, const std::vector<_Float16>& pk, uint4** dst) {
  HIP_TRY(h, dalloc(dst, pk.size() / 8));
  HIP_TRY(h, hipMemcpy(*dst, pk.data(), pk.size() * sizeof(_Float16), hipMemcpyHostToDevice));
  return SN_OK;
}

// 2-D conv weights [co][ci][ky][kx] -> packed [ci_pad][tap][co]
int upload_conv2d(sn_handle* h, const HostLayer& l, int ch_multiple, ConvLayer* out) {
  const int cin_pad = (l.cin + ch_multiple - 1) / ch_multiple * ch_multiple;
  std::vector<float> pk((size_t)cin_pad * l.taps * kC, 0.f);
  for (int co = 0; co < kC; ++co)
    for (int ci = 0; ci < l.cin; ++ci)
      for (int t = 0; t < l.taps; ++t)
        pk[((size_t)ci * l.taps + t) * kC + co] = l.w[((size_t)co * l.cin + ci) * l.taps + t];
  out->cin = l.cin;
  out->cin_pad = cin_pad;
  out->taps = l.taps;
  const int rc = to_device(h, pk.data(), pk.size(), &out->wpk);
  return rc ? rc : to_device(h, l.b, kC, &out->bias);
}

// 3-D conv weights [co][ci][kz][ky][kx] -> packed [c' = kz*32+ci][tap = ky*3+kx][co]  (96 virtual channels)
int upload_conv3d(sn_handle* h, const HostLayer& l, ConvLayer* out) {
  std::vector<float> pk((size_t)96 * 9 * kC, 0.f);
  for (int co = 0; co < kC; ++co)
    for (int ci = 0; ci < kC; ++ci)
      for (int kz = 0; kz < 3; ++kz)
        for (int t = 0; t < 9; ++t)
          pk[((size_t)(kz * kC + ci) * 9 + t) * kC + co] = l.w[(((size_t)co * kC + ci) * 3 + kz) * 9 + t];
  out->cin = 96;
  out->cin_pad = 96;
  out->taps = 9;
  const int rc = to_device(h, pk.data(), pk.size(), &out->wpk);
  return rc ? rc : to_device(h, l.b, kC, &out->bias);
}

// split fp16 A-fragments for k_conv3x3_c32_x3: wv(co, c', tap) is the weight of virtual input channel c'
template <class WV>
int upload_x3(sn_handle* h, int cin_virtual, WV wv, ConvLayer* out, int taps = 9, bool zero_lo = false) {
  const int nchunk = cin_virtual / 16;
  std::vector<_Float16> pk((size_t)nchunk * taps * 2 * 64 * 8);
  for (int ch = 0; ch < nchunk; ++ch)
    for (int tap = 0; tap < taps; ++tap)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) {
          const int co = lane & 31, c = ch * 16 + 8 * (lane >> 5) + e;
          const float w = wv(co, c, tap);
          const _Float16 hi = (_Float16)w;
          const size_t base = (((size_t)ch * taps + tap) * 2) * 64 * 8 + (size_t)lane * 8 + e;
          pk[base] = hi;
          pk[base + 64 * 8] = zero_lo ? (_Float16)0.f : (_Float16)((w - (float)hi) * kSplitScale);
        }
  return to_device(h, pk, &out->wx3);
}

// A-fragments of k_down0_f16: K = 8 * rho + kx, rho = ci * 5 + ky (row 15 and kx >= 5 are zero)
int upload_down0_f16(sn_handle* h, const HostLayer& l, Down0F16* out) {
  std::vector<_Float16> pk((size_t)8 * 2 * 64 * 8);
  for (int t = 0; t < 8; ++t)
    for (int lane = 0; lane < 64; ++lane)
      for (int e = 0; e < 8; ++e) {
        const int co = lane & 31, rho = 2 * t + (lane >> 5);
        const float w = (rho < 15 && e < 5) ? l.w[((size_t)co * 3 + rho / 5) * 25 + (rho % 5) * 5 + e] : 0.f;
        const _Float16 hi = (_Float16)w;
        const size_t base = ((size_t)(2 * t) * 64 + lane) * 8 + e;
        pk[base] = hi;
        pk[base + 64 * 8] = (_Float16)((w - (float)hi) * kSplitScale);
      }
  return to_device(h, pk, &out->wfrag);
}

// A-fragments of k_refin_f16: K = 8 * tap + e over the pixel slot [d_hi, Y_hi, U_hi, V_hi, d_lo, Y_lo, U_lo, V_lo]
// (the image lo parts are zero when the source is the int8 model input, whose values are exact in fp16);
// fragment a = hi weights on entries 0..3; fragment b = lo weights on entries 0..3 + hi weights on entries 4..7
int upload_refin_f16(sn_handle* h, const HostLayer& l, Down0F16* out) {
  std::vector<_Float16> pk((size_t)5 * 2 * 64 * 8, (_Float16)0.f);
  for (int t = 0; t < 5; ++t)
    for (int lane = 0; lane < 64; ++lane) {
      const int co = lane & 31, tap = 2 * t + (lane >> 5);
      if (tap >= 9) continue;
      _Float16* a = &pk[((size_t)(2 * t) * 64 + lane) * 8];
      _Float16* b = a + 64 * 8;
      for (int c = 0; c < 4; ++c) {
        const float w = l.w[((size_t)co * 4 + c) * 9 + tap];
        const _Float16 hi = (_Float16)w;
        a[c] = hi;
        b[c] = (_Float16)((w - (float)hi) * kSplitScale);
        b[4 + c] = hi;
      }
    }
  return to_device(h, pk, &out->wfrag);
}
int upload_down01(sn_handle* h, const HostLayer& l0, const HostLayer& l1, Down01W* out) {
  std::vector<double> weff, beff;
  compose_down01(l0.w, l0.b, l1.w, l1.b, weff, beff);
  std::vector<_Float16> pk;
  pack_down01(weff, pk);
  std::vector<float> bf(beff.begin(), beff.end());
  const int rc = to_device(h, pk, &out->wfrag);
  return rc ? rc : to_device(h, bf.data(), bf.size(), &out->bias);
}

int upload_head(sn_handle* h, const HostLayer& l, HeadLayer* out) {   // [1][32][taps] as-is
  out->bias = l.b[0];
  return to_device(h, l.w, (size_t)kC * l.taps, &out->w);
}

// ref*.out for the head kernels of the fp16 modes (HeadLayer::wsplit): the power of two that brings the largest |w| into
// [1/2, 1) when it is below 2^-12, none otherwise (a model that is fine today computes what it did, bit for bit).  Measured
// reason (tests/test_gpu_truth64_range.py, profiles/activation_range.txt): a tower gauged by 2^12 has head weights of 6e-8, one
// fp16 subnormal step, and SN_PREC_F16X3 showed a coherent 3.8e-5 px offset there.
int upload_head_split(sn_handle* h, const HostLayer& l, HeadLayer* out) {
  int rc = upload_head(h, l, out);
  if (rc) return rc;
  const size_t n = (size_t)kC * l.taps;
  float top = 0.f;
  for (size_t i = 0; i < n; ++i) top = fabsf(l.w[i]) > top ? fabsf(l.w[i]) : top;
  out->wsplit = out->w;
  out->biassplit = out->bias;
  out->unscale = 1.f;
  if (!(top > 0.f) || !(top < 0x1p-12f) || !std::isfinite(top)) return SN_OK;
  int e = 0;
  (void)frexpf(top, &e);                 // top = m * 2^e, m in [1/2, 1)
  const float up = ldexpf(1.f, -e);
  if (!std::isfinite(out->bias * up) || !std::isfinite(up)) return SN_OK;     // (a bias that large next to weights that small: leave it)
  std::vector<float> ws(n);
  for (size_t i = 0; i < n; ++i) ws[i] = l.w[i] * up;
  out->biassplit = out->bias * up;
  out->unscale = ldexpf(1.f, e);
  return to_device(h, ws.data(), n, &out->wsplit);
}

// agg.out as the A operand of P[tap][pixel] = sum_c w[c][tap] y[c][pixel] (k_agg_x3s_dma<false, true>): row m = tap
// (27 of 32 rows), K-step kk = channels 16 kk .. 16 kk + 15, lane (m, g) holds channels 16 kk + 8 g + e; hi / lo split
int upload_agg_head_frag(sn_handle* h, const HostLayer& l, HeadLayer* out) {
  std::vector<_Float16> pk((size_t)2 * 2 * 64 * 8, (_Float16)0.f);
  for (int kk = 0; kk < 2; ++kk)
    for (int lane = 0; lane < 64; ++lane)
      for (int e = 0; e < 8; ++e) {
        const int m = lane & 31, c = 16 * kk + 8 * (lane >> 5) + e;
        if (m >= 27) continue;
        const float w = l.w[(size_t)c * 27 + m];
        const _Float16 hi = (_Float16)w;
        const size_t base = ((size_t)(2 * kk) * 64 + lane) * 8 + e;
        pk[base] = hi;
        pk[base + 64 * 8] = (_Float16)((w - (float)hi) * kSplitScale);
      }
  return to_device(h, pk, &out->pfrag);
}

// ---- fp16 weights of the tower (SN_PREC_F16): sum-preserving rounding of every 3x3 kernel ----------------------------
// Rounding each weight to nearest leaves every (cout, cin) kernel with a sum error of ~sqrt(9) half-ulps.  The tower's
// activations are LeakyReLU outputs: positive mean, and smooth wherever the image is — so a kernel's response to them is
// mostly (sum of its taps) x (local mean), and the sum errors of the 32 x 32 x 12 kernels add up COHERENTLY over the whole
// image into an offset of the refinement residual: 2.4e-4 ... 1.1e-3 px at D = 192 depending on the weight draw and the
// image content, the largest single term of the mode's error (scripts/f16_error_sources.py,
// profiles/r05_f16_error_sources.txt).  Here each kernel's nine taps are rounded down or up (never further than the two
// neighbouring fp16 numbers) in the combination, out of the 512, whose SUM of errors is smallest: the offset disappears
// (< 2e-5 px in the same experiment), at the price of individual tap errors of up to one ulp instead of half — which only
// the high-frequency part of the activations sees.  Costs nothing at run time, needs no calibration data; weights that
// are exact in fp16 stay as they are.  SN_W_ROUND=rne restores round-to-nearest (A/B switch).
inline _Float16 f16_neighbour(_Float16 hval, bool up) {
  uint16_t b;
  memcpy(&b, &hval, 2);
  if (up) {
    if (b == 0x8000) b = 0x0001;
    else if (b & 0x8000) b -= 1;
    else b += 1;
  } else {
    if (b == 0x0000) b = 0x8001;
    else if (b & 0x8000) b += 1;
    else b -= 1;
  }
  _Float16 r;
  memcpy(&r, &b, 2);
  return r;
}

// w[9] -> q[9]: q[t] is one of the two fp16 numbers enclosing w[t]
void round_kernel_sum_preserving(const float* w, _Float16* q) {
  double lo[9], hi[9];
  _Float16 hlo[9], hhi[9];
  for (int t = 0; t < 9; ++t) {
    const _Float16 n = (_Float16)w[t];
    const double nd = (double)n, wd = (double)w[t];
    hlo[t] = nd <= wd ? n : f16_neighbour(n, false);
    hhi[t] = nd >= wd ? n : f16_neighbour(n, true);
    lo[t] = (double)hlo[t] - wd;        // <= 0
    hi[t] = (double)hhi[t] - wd;        // >= 0
  }
  int best = 0;
  double best_score = 1e300;
  for (int m = 0; m < 512; ++m) {
    double sum = 0, sq = 0;
    for (int t = 0; t < 9; ++t) {
      const double e = (m >> t) & 1 ? hi[t] : lo[t];
      sum += e;
      sq += e * e;
    }
    const double score = std::fabs(sum) + 1e-3 * std::sqrt(sq);      // sum first; among (near-)ties the smallest errors
    if (score < best_score) {
      best_score = score;
      best = m;
    }
  }
  for (int t = 0; t < 9; ++t) q[t] = (best >> t) & 1 ? hhi[t] : hlo[t];
}

// sp: Switches::w_round_sum_preserving as read by the caller (sn_create, or a parity hook at the time it is called)
int upload_ref_f16(sn_handle* h, const HostLayer& l, bool sp, RefLayerF16* out) {
  std::vector<_Float16> q((size_t)kC * kC * 9);
  for (size_t k = 0; k < (size_t)kC * kC; ++k) {
    if (sp) {
      round_kernel_sum_preserving(l.w + k * 9, &q[k * 9]);
    } else {
      for (int t = 0; t < 9; ++t) q[k * 9 + t] = (_Float16)l.w[k * 9 + t];
    }
  }
  std::vector<_Float16> pk((size_t)18 * 64 * 8);
  for (int tap = 0; tap < 9; ++tap)
    for (int kk = 0; kk < 2; ++kk)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) {
          const int co = lane & 31, ci = 16 * kk + 8 * (lane >> 5) + e;
          pk[(((size_t)tap * 2 + kk) * 64 + lane) * 8 + e] = q[((size_t)co * kC + ci) * 9 + tap];
        }
  const int rc = to_device(h, pk, &out->wfrag);
  return rc ? rc : to_device(h, l.b, kC, &out->bias);
}

// F16X3: [co][ci][ky][kx] fp32 -> hi fragments (18 x 64 slots) followed by lo fragments, lo = fp16((w - hi) * 2^11)
int upload_ref_f16x3(sn_handle* h, const HostLayer& l, RefLayerF16* out) {
  std::vector<_Float16> pk((size_t)36 * 64 * 8);
  for (int tap = 0; tap < 9; ++tap)
    for (int kk = 0; kk < 2; ++kk)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) {
          const int co = lane & 31, ci = 16 * kk + 8 * (lane >> 5) + e;
          const float w = l.w[((size_t)co * kC + ci) * 9 + tap];
          const _Float16 hi = (_Float16)w;
          const size_t i = (((size_t)tap * 2 + kk) * 64 + lane) * 8 + e;
          pk[i] = hi;
          pk[(size_t)18 * 64 * 8 + i] = (_Float16)((w - (float)hi) * kSplitScale);
        }
  const int rc = to_device(h, pk, &out->wfrag);
  return rc ? rc : to_device(h, l.b, kC, &out->bias);
}

}  // namespace
