// sn_launch.hpp — one launcher per kernel (grid, LDS size and argument block from the tensor geometry), the per-layer
// dispatchers built on them (conv3x3, conv5x5s2, ref_conv_f16*, ref_block_*), and the geometry of the padded tensors the
// kernels read (make_ref_geom, ref_slack, ref_front, alloc_ref16, vol_pad, feat_pad, down_in_geom).  Nothing here knows
// about the handle or the order of the forward pass.  Part of the single translation unit stereonet_hip.hip.
#pragma once

namespace {

// Raise a kernel's dynamic-LDS limit once per (kernel, device) — not per launch: launches may happen inside a
// stream capture.  Keyed by the kernel's address (different instantiations can share one function type).
template <class K>
hipError_t ensure_lds_attr(K kern, int bytes) {
  static std::mutex mu;
  static std::unordered_map<const void*, unsigned long long> done;     // kernel -> bitmask of device ordinals
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  const unsigned long long bit = 1ull << (dev & 63);
  const void* key = reinterpret_cast<const void*>(kern);
  std::lock_guard<std::mutex> lk(mu);
  unsigned long long& m = done[key];
  if (m & bit) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(key, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) m |= bit;
  return e;
}

// Argument block of the ConvArgs kernels: layer L (w: the weight form the kernel reads), out / res tensors, nimg images of
// Ho x Wo outputs in TR x TC tiles.
inline ConvArgs make_conv_args(const ConvLayer& L, const void* w, void* out, const void* res, int nimg, int Ho, int Wo, int dil,
                               int pad, bool lrelu, int TR, int TC) {
  ConvArgs a{};
  a.wpk = reinterpret_cast<const float*>(w);
  a.bias = L.bias;
  a.out = reinterpret_cast<float*>(out);
  a.res = reinterpret_cast<const float*>(res);
  a.nimg = nimg;
  a.cin_pad = L.cin_pad;
  a.Ho = Ho;
  a.Wo = Wo;
  a.dil = dil;
  a.pad = pad;
  a.lrelu = lrelu ? 1 : 0;
  a.tiles_x = (Wo + TC - 1) / TC;
  a.tiles_y = (Ho + TR - 1) / TR;
  return a;
}

// the launchers' optional report (LaunchInfo, sn_engine.hpp)
inline void report(LaunchInfo* li, int wgs, int units) {
  if (li) *li = LaunchInfo{wgs, units};
}

// Persistent grid of at most `cap` workgroups over `total` tiles, a multiple of 8: one band of tiles per XCD.
inline int xcd_band_grid(int cap, int total) {
  const int need = (total + 7) / 8 * 8;
  return ((cap > need ? need : cap) + 7) / 8 * 8;
}

// img_src: the int8 model input [n][6][H][W] (pyr = false) or the float image pyramid level [n][3][g.H][g.W].
template <int TW>
hipError_t launch_refin_f16_tw(hipStream_t st, const Down0F16& L, const float* bias, const float* disp_low,
                               const void* img_src, bool pyr, int hl, int wl, int H, int W, float inv_d, UpScale ups,
                               RefGeom g, int nimg, uint4* out, bool split, size_t lo_off_bytes, int num_cu,
                               LaunchInfo* li = nullptr) {
  using T = RefInTile<TW>;
  g.tiles_x = (g.W + TW - 1) / TW;
  g.tiles_y = (g.H + T::TH - 1) / T::TH;
  const int total = g.tiles_x * g.tiles_y * nimg;
  int blocks = 2 * num_cu;
  if (blocks > total) blocks = total;
  report(li, blocks, total);
  const int al4 = !pyr && (W % 4 == 0) && (reinterpret_cast<uintptr_t>(img_src) % 4 == 0);
#define SN_REFIN(S, P)                                                                                             \
  hipLaunchKernelGGL((k_refin_f16<S, P, TW>), dim3(blocks), dim3(256), T::LDS_BYTES, st, disp_low, img_src, hl, wl, H, \
                     W, inv_d, ups, L.wfrag, bias, out, lo_off_bytes, g, nimg, al4)
  if (split && pyr) SN_REFIN(true, true);
  else if (split) SN_REFIN(true, false);
  else if (pyr) SN_REFIN(false, true);
  else SN_REFIN(false, false);
#undef SN_REFIN
  return hipGetLastError();
}

// (8x32 tiles, which pay off for the tower's dilation-1 / -2 launches, were measured for this kernel too: 54.8 us
// against 41.5 us per two pairs at 1280x720 — only 100 of the 256 threads have a staging unit then.)
hipError_t launch_refin_f16(hipStream_t st, const Down0F16& L, const float* bias, const float* disp_low,
                            const void* img_src, bool pyr, int hl, int wl, int H, int W, float inv_d, UpScale ups,
                            const RefGeom& g, int nimg, uint4* out, bool split, size_t lo_off_bytes, int num_cu,
                            LaunchInfo* li = nullptr) {
  return launch_refin_f16_tw<64>(st, L, bias, disp_low, img_src, pyr, hl, wl, H, W, inv_d, ups, g, nimg, out, split,
                                 lo_off_bytes, num_cu, li);
}

hipError_t launch_down0_f16(hipStream_t st, const Down0F16& L, const float* bias, const int8_t* in6, int H, int W,
                            int nimg, int Ho, int Wo, float* out, int num_cu, const SlotGeom* og = nullptr,
                            LaunchInfo* li = nullptr) {
  constexpr int TC = 32;
  using T = Down0Tile<TC>;
  const int tiles_x = (Wo + TC - 1) / TC, tiles_y = (Ho + T::TR - 1) / T::TR;
  const int total = tiles_x * tiles_y * nimg;
  int blocks = 2 * num_cu;                        // register budget: two workgroups per CU
  if (blocks > total) blocks = total;
  report(li, blocks, total);
  const int al4 = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(in6) % 4 == 0);
  hipLaunchKernelGGL((k_down0_f16<TC>), dim3(blocks), dim3(256), T::LDS_BYTES, st, in6, H, W, L.wfrag, bias, out, Ho, Wo,
                     tiles_x, tiles_y, nimg, 0, al4, og ? og->PH : Ho, og ? og->PW : Wo, og ? og->py : 0, og ? og->px : 0);
  return hipGetLastError();
}

// in6: int8 model input of the piece; out: split-slot tensor of the quarter-resolution map in geometry `og`
// (W4: dword loads at any byte address — the int8 planes need no alignment, only W % 4 decides which instance runs)
template <bool W4>
hipError_t launch_down01_w(hipStream_t st, const Down01W& L, const int8_t* in6, int H, int W, int nimg, int Ho, int Wo,
                           uint4* out, const SlotGeom& og, int num_cu, LaunchInfo* li = nullptr) {
  using T = Down01;
  hipError_t e = ensure_lds_attr(k_down01_f16<W4>, T::LDS_BYTES);
  if (e != hipSuccess) return e;
  const int tiles_x = (Wo + T::TC - 1) / T::TC, tiles_y = (Ho + T::TR - 1) / T::TR;
  const int total = tiles_x * tiles_y * nimg;
  int blocks = num_cu / 8 * 8;                    // one workgroup per CU (register budget), whole XCD bands
  while (blocks > 8 && blocks / 8 > (total + 7) / 8) blocks -= 8;
  report(li, blocks, total);
  hipLaunchKernelGGL(k_down01_f16<W4>, dim3(blocks), dim3(256), T::LDS_BYTES, st, in6, H, W,
                     L.wfrag + (size_t)T::INNER * T::NK * 2 * 64, L.bias + T::INNER * kC, out, Ho, Wo, tiles_x, tiles_y, nimg,
                     og.PH, og.PW, og.py, og.px);
  const int per_img = 4 + 2 * ((Wo - 2 + 31) / 32) + 2 * ((Ho - 2 + 31) / 32);
  hipLaunchKernelGGL(k_down01_border<W4>, dim3(per_img * (nimg / 2)), dim3(192), 0, st, in6, H, W, L.wfrag, L.bias, out,
                     Ho, Wo, nimg, og.PH, og.PW, og.py, og.px);
  return hipGetLastError();
}
hipError_t launch_down01(hipStream_t st, const Down01W& L, const int8_t* in6, int H, int W, int nimg, int Ho, int Wo,
                         uint4* out, const SlotGeom& og, int num_cu, LaunchInfo* li = nullptr) {
  return (W % 4) == 0 ? launch_down01_w<true>(st, L, in6, H, W, nimg, Ho, Wo, out, og, num_cu, li)
                      : launch_down01_w<false>(st, L, in6, H, W, nimg, Ho, Wo, out, og, num_cu, li);
}

// weights-stationary split-operand conv on split-slot tensors: persistent grid of MINB workgroups per CU
template <int KS, int STRIDE, int VCH, int TR, int TC, int SEGW, int MINB, bool OUTSLOT, class Loader, bool HASRES = false>
hipError_t launch_conv_x3s(hipStream_t st, const ConvLayer& L, const Loader& ld, int nimg, int Ho, int Wo, float* out,
                           const float* res, bool lrelu, int num_cu, LaunchInfo* li = nullptr) {
  using T = X3sTile<KS, STRIDE, VCH, TR, TC, SEGW>;
  const ConvArgs a = make_conv_args(L, L.wx3, out, res, nimg, Ho, Wo, 1, KS / 2, lrelu, TR, TC);
  if (res != nullptr && !HASRES)      // residual layers use their own instantiation (16 more registers)
    return launch_conv_x3s<KS, STRIDE, VCH, TR, TC, SEGW, MINB, OUTSLOT, Loader, true>(st, L, ld, nimg, Ho, Wo, out, res, lrelu, num_cu, li);
  auto kern = k_conv_x3s<KS, STRIDE, VCH, TR, TC, SEGW, MINB, OUTSLOT, HASRES, Loader>;
  static_assert(T::LDS_BYTES <= 160 * 1024, "x3s tile does not fit the LDS");
  if (T::LDS_BYTES > 64 * 1024) {
    hipError_t e = ensure_lds_attr(kern, (int)T::LDS_BYTES);
    if (e != hipSuccess) return e;
  }
  const int blocks = xcd_band_grid(num_cu * MINB, a.tiles_x * a.tiles_y * nimg);
  report(li, blocks, a.tiles_x * a.tiles_y * nimg);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), T::LDS_BYTES, st, a, ld);
  return hipGetLastError();
}

// ---- precision ablation of the low-resolution branch (scripts/lowres_ablation.py) -------------------------------------
// DIAGNOSTIC BUILD ONLY (-DSN_DIAGNOSTICS=1: `python -m hobot_stereonet_amd.build --diag` -> libstereonet_hip_diag.so, which the
// script loads through STEREONET_HIP_LIB); the shipping library ignores both variables (sn_switches.hpp parses them).
// The split-operand layers evaluate x*w as xh*wh + (xh*wl + xl*wh) / 2048 (three fp16 MFMAs).  What a cheaper form of a
// layer would compute is reproduced exactly with zeroed operands (an MFMA with a zero operand adds exact zeros):
//   SN_ABLATE_W=<layers>  the layer's weights rounded to fp16: its lo A-fragments are uploaded as zeros  (drops xh*wl)
//   SN_ABLATE_X=<layers>  the layer's input rounded to fp16: the lo slots of its input tensor are zeroed in front of the
//                         launch (drops xl*wh; runs the plain split-slot layouts, which are bit-identical to the
//                         zero-bordered ones; for the first conv of a residual block the rounded tensor is also the
//                         block's residual input, so that entry is an upper bound)
#if !SN_DIAGNOSTICS
inline hipError_t zero_lo_slots(hipStream_t, float*, int, size_t) { return hipSuccess; }
#else
// split-slot tensor [nblk][hi | lo][hw] (nblk = images x 4 channel blocks): zero the lo halves
__global__ void k_zero_lo_slots(uint4* t, size_t hw, size_t nblk) {
  const size_t total = nblk * hw;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t b = i / hw, r = i - b * hw;
    t[(2 * b + 1) * hw + r] = uint4{0u, 0u, 0u, 0u};
  }
}
inline hipError_t zero_lo_slots(hipStream_t st, float* tensor, int nimg, size_t hw) {
  hipLaunchKernelGGL(k_zero_lo_slots, dim3(1024), dim3(256), 0, st, reinterpret_cast<uint4*>(tensor), hw, (size_t)nimg * 4);
  return hipGetLastError();
}
#endif      // SN_DIAGNOSTICS

VolPad vol_pad(int Dl, int hl, int wl) { return VolPad{Dl, hl, wl, VolPad::ph(hl), VolPad::pw(wl)}; }

// 3x3x3 aggregation layer on zero-bordered split-slot volumes (sn_agg_dma.hpp): one persistent workgroup per CU
// head_frag != nullptr (OUTSLOT = false): the layer ends in the output conv's taps-as-M contraction and writes its partial
// sums P [npairs Dl][27][H][W] instead of the activated volume (k_agg_x3s_dma HEADP)
template <bool OUTSLOT, bool HEADP = false>
hipError_t launch_agg_dma(hipStream_t st, const ConvLayer& L, const uint4* vin, const VolPad& g, int npairs, void* out,
                          bool lrelu, int num_cu, const uint4* head_frag = nullptr, LaunchInfo* li = nullptr) {
  if (HEADP != (head_frag != nullptr)) return hipErrorInvalidValue;
  const ConvArgs a = make_conv_args(L, L.wx3, out, head_frag, npairs * g.Dl, g.H, g.W, 1, 1, lrelu, 8, 16);
  auto kern = k_agg_x3s_dma<OUTSLOT, HEADP>;
  hipError_t e = ensure_lds_attr(kern, (int)AggDma::LDS_BYTES);
  if (e != hipSuccess) return e;
  const int blocks = xcd_band_grid(num_cu, a.tiles_x * a.tiles_y * a.nimg);
  report(li, blocks, a.tiles_x * a.tiles_y * a.nimg);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), AggDma::LDS_BYTES, st, a, vin, g);
  return hipGetLastError();
}

FeatPad feat_pad(int H, int W) { return FeatPad{H, W, FeatPad::ph(H), FeatPad::pw(W)}; }

// 3x3 32->32 feature layer on zero-bordered split-slot tensors (sn_feat_dma.hpp): two persistent workgroups per CU.
// out / res: FeatPad tensors (OUTSLOT) or fp32 NCHW.
template <bool OUTSLOT, bool HASRES>
hipError_t launch_feat_dma(hipStream_t st, const ConvLayer& L, const uint4* vin, const FeatPad& g, int nimg, void* out,
                           const void* res, bool lrelu, int num_cu, LaunchInfo* li = nullptr) {
  const ConvArgs a = make_conv_args(L, L.wx3, out, res, nimg, g.H, g.W, 1, 1, lrelu, 8, 16);
  auto kern = k_feat_x3s_dma<OUTSLOT, HASRES>;
  hipError_t e = ensure_lds_attr(kern, (int)FeatDma::LDS_BYTES);
  if (e != hipSuccess) return e;
  const int blocks = xcd_band_grid(2 * num_cu, a.tiles_x * a.tiles_y * a.nimg);
  report(li, blocks, a.tiles_x * a.tiles_y * a.nimg);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), FeatDma::LDS_BYTES, st, a, vin, g);
  return hipGetLastError();
}

// zero-bordered input grid of a 5x5 stride-2 down-conv with an Ho x Wo output
SlotGeom down_in_geom(int Ho, int Wo) { return SlotGeom{DownDma::ph(Ho), DownDma::pw(Wo), DownDma::PADY, DownDma::PADX}; }

// 5x5 stride-2 32->32 down-conv on a zero-bordered split-slot input (sn_agg_dma.hpp); go = the output tensor's grid
hipError_t launch_down_dma(hipStream_t st, const ConvLayer& L, const uint4* vin, int nimg, int Ho, int Wo, void* out,
                           const SlotGeom& go, bool lrelu, int num_cu, LaunchInfo* li = nullptr) {
  const ConvArgs a = make_conv_args(L, L.wx3, out, nullptr, nimg, Ho, Wo, 1, 2, lrelu, DownDma::TR, DownDma::TC);
  hipError_t e = ensure_lds_attr(k_down_x3s_dma, (int)DownDma::LDS_BYTES);
  if (e != hipSuccess) return e;
  const int blocks = xcd_band_grid(num_cu, a.tiles_x * a.tiles_y * nimg);
  report(li, blocks, a.tiles_x * a.tiles_y * nimg);
  hipLaunchKernelGGL(k_down_x3s_dma, dim3(blocks), dim3(256), DownDma::LDS_BYTES, st, a, vin, down_in_geom(Ho, Wo), go);
  return hipGetLastError();
}

// ---- convolution launcher ------------------------------------------------------------------------
template <int KS, int STRIDE, int DIL, int CH, int TR, int TC, class Loader, bool PF = true, int MINW = 1>
hipError_t launch_conv(hipStream_t st, const ConvLayer& L, const Loader& ld, int nimg, int Ho, int Wo,
                       float* out, const float* res, bool lrelu) {
  constexpr int dil = DIL;
  const ConvArgs a = make_conv_args(L, L.wpk, out, res, nimg, Ho, Wo, dil, (KS / 2) * dil, lrelu, TR, TC);
  const int rows_in = (TR - 1) * STRIDE + (KS - 1) * dil + 1;
  const int cols_in = (TC - 1) * STRIDE + (KS - 1) * dil + 1;
  const int pitch = STRIDE == 1 ? cols_in : 2 * ((cols_in + 1) / 2);
  const size_t lds = ((size_t)CH * KS * KS * 32 + (size_t)CH * rows_in * pitch) * sizeof(float);
  auto kern = k_conv_c32_mfma<KS, STRIDE, DIL, CH, TR, TC, Loader, PF, MINW>;
  if (lds > 64 * 1024) {
    hipError_t e = ensure_lds_attr(kern, (int)lds);
    if (e != hipSuccess) return e;
  }
  const int nwg = a.tiles_x * a.tiles_y * nimg;
  hipLaunchKernelGGL(kern, dim3(nwg), dim3(256), lds, st, a, ld);
  return hipGetLastError();
}

// 3x3 C->C conv on a plain NCHW fp32 tensor; tile shape chosen from image size and dilation
template <int DIL>
hipError_t conv3x3_d(hipStream_t st, const ConvLayer& L, const float* in, int nimg, int H, int W, float* out,
                     const float* res, bool lrelu) {
  LoadF32 ld{in, kC, H, W};
  // (chunk sizes 8/16 and tile heights 4/8 measured equal within noise on the 45x80 low-resolution maps)
  if (H * W <= 64 * 128) return launch_conv<3, 1, DIL, 8, 4, 32>(st, L, ld, nimg, H, W, out, res, lrelu);
  if (DIL >= 4) return launch_conv<3, 1, DIL, 4, 16, 64>(st, L, ld, nimg, H, W, out, res, lrelu);
  return launch_conv<3, 1, DIL, 8, 8, 64>(st, L, ld, nimg, H, W, out, res, lrelu);
}

// Tower layers of SN_PREC_FP32 (plain fp32 NCHW, 32 -> 32, 3x3 dilated): the weights-stationary kernel of sn_tower_f32.hpp.
template <int DIL, int CPH, int NW = 8>
hipError_t launch_ref_conv_f32(hipStream_t st, const ConvLayer& L, const float* in, int nimg, int H, int W, float* out,
                               const float* res, bool lrelu, int num_cu, LaunchInfo* li = nullptr) {
  using T = F32Tile<DIL, CPH, 64, NW>;
  auto kern = res ? k_ref_conv_f32<DIL, CPH, true, NW> : k_ref_conv_f32<DIL, CPH, false, NW>;
  if (T::LDS_BYTES > 64 * 1024 - 1024) {
    hipError_t e = ensure_lds_attr(kern, T::LDS_BYTES);
    if (e != hipSuccess) return e;
  }
  const int total = ((W + T::TW - 1) / T::TW) * ((H + T::TH - 1) / T::TH) * nimg;
  // persistent: ONE workgroup per CU (it double-buffers its own staging, sn_tower_f32.hpp), each walks a contiguous share of
  // the launch's HALF tiles (1280x720, one pair = 3600 halves on 256 CUs = 14.06 per workgroup instead of 8 whole tiles for
  // 7.03 tiles of work)
  int grid = 2 * total < num_cu ? 2 * total : num_cu;
  const int grid_env = switches().f32_grid;          // probe: workgroups per launch
  if (grid_env > 0) grid = grid_env < 2 * total ? grid_env : 2 * total;
  if (grid < 1) grid = 1;
  report(li, grid, 2 * total);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NW), T::LDS_BYTES, st, in, out, res, L.wpk, L.bias, nimg, H, W, lrelu ? 1 : 0);
  return hipGetLastError();
}

hipError_t conv3x3(hipStream_t st, const ConvLayer& L, const float* in, int nimg, int H, int W, int dil,
                   float* out, const float* res, bool lrelu, int tower_cu = 0, LaunchInfo* li = nullptr) {
  // (the 16-byte staging wants rows that start 16-byte aligned: W % 4 == 0 — every level-0 geometry, not every coarse
  // level of a hierarchical model)
  if (tower_cu > 0 && L.cin == kC && L.cin_pad == kC && (W & 3) == 0 && switches().f32_tower) {      // SN_F32_TOWER=0 keeps the generic kernel (A/B)
    switch (dil) {
      case 1: return launch_ref_conv_f32<1, 8>(st, L, in, nimg, H, W, out, res, lrelu, tower_cu, li);
      case 2: return launch_ref_conv_f32<2, 8>(st, L, in, nimg, H, W, out, res, lrelu, tower_cu, li);
      case 4: return launch_ref_conv_f32<4, 4, 16>(st, L, in, nimg, H, W, out, res, lrelu, tower_cu, li);
      // dilation 4 / 8: sixteen rows per tile (1024 threads) — 16 / 24 halo rows per 8 would be 2 - 3x the staging of the tile itself
      case 8: return launch_ref_conv_f32<8, 4, 16>(st, L, in, nimg, H, W, out, res, lrelu, tower_cu, li);
      default: return hipErrorInvalidValue;
    }
  }
  switch (dil) {
    case 1: return conv3x3_d<1>(st, L, in, nimg, H, W, out, res, lrelu);
    case 2: return conv3x3_d<2>(st, L, in, nimg, H, W, out, res, lrelu);
    case 4: return conv3x3_d<4>(st, L, in, nimg, H, W, out, res, lrelu);
    case 8: return conv3x3_d<8>(st, L, in, nimg, H, W, out, res, lrelu);
    default: return hipErrorInvalidValue;
  }
}

hipError_t conv5x5s2(hipStream_t st, const ConvLayer& L, const float* in, int nimg, int Hin, int Win,
                     float* out) {
  LoadF32 ld{in, kC, Hin, Win};
  const int Ho = Hin / 2, Wo = Win / 2;
  // 8 x 64 tiles are the efficient shape, but a launch needs workgroups: a single pair's second down-conv is 56 of them on
  // 256 CUs (130 us for a quarter of the first one's work, profiles/r05_fp32_b1_kernel_summary.txt); below two workgroups
  // per CU the 4 x 32 shape (same K order, same sums) fills the chip instead
  const long big_tiles = (long)((Wo + 63) / 64) * ((Ho + 7) / 8) * nimg;
  if (Ho * Wo <= 64 * 128 || big_tiles < 512) return launch_conv<5, 2, 1, 4, 4, 32>(st, L, ld, nimg, Ho, Wo, out, nullptr, false);
  return launch_conv<5, 2, 1, 4, 8, 64>(st, L, ld, nimg, Ho, Wo, out, nullptr, false);
}

// ---- fp16 refinement tower -------------------------------------------------------------------------
RefGeom make_ref_geom(int Hp, int Wp) {
  RefGeom g{};
  g.tiles_x = (Wp + 63) / 64;
  g.tiles_y = (Hp + 7) / 8;
  g.H = Hp;
  g.W = Wp;
  g.Hs = (Hp + 15) / 16 * 16 + 2 * kRefPad;      // whole 16-row tiles (tall-tile variants of the dilated layers)
  g.Ws = g.tiles_x * 64 + 2 * kRefPad;
  return g;
}

size_t ref16_slots(const RefGeom& g, int nimg) { return (size_t)nimg * 4 * g.Hs * g.Ws; }
// The streaming block kernels the pipeline instantiates (ref_block_stream below): ONE list, from which the zero rows
// around a tensor are derived.
using StreamTile1 = StreamTile<1, 64, 4, 6, 4>;
using StreamTile2 = StreamTile<2, 64, 4, 6, 4>;
using StreamTile4 = StreamTile<4, 128, 2, 6, 4>;
using StreamTile8 = StreamTile<8, 128, 2, 6, 4>;
using StreamTileTail = StreamTile<1, 64, 4, 5, 4, true>;      // last block + refinement head (x ring of 5 groups: early residual fetch)
static_assert(StreamTileTail::ROWS_ABOVE <= kRefPad && StreamTileTail::ROWS_BELOW <= StreamTile8::ROWS_BELOW, "tail form stays inside the zero rows");
constexpr int cmax4(int a, int b, int c, int d) { return (a > b ? a : b) > (c > d ? c : d) ? (a > b ? a : b) : (c > d ? c : d); }
constexpr int kStreamRowsAbove = cmax4(StreamTile1::ROWS_ABOVE, StreamTile2::ROWS_ABOVE, StreamTile4::ROWS_ABOVE, StreamTile8::ROWS_ABOVE);
constexpr int kStreamRowsBelow = cmax4(StreamTile1::ROWS_BELOW, StreamTile2::ROWS_BELOW, StreamTile4::ROWS_BELOW, StreamTile8::ROWS_BELOW);
// Slots behind a tensor that kernels may over-read (never written, zero).  Streaming kernel: a DMA group reaches up to
// ROWS_BELOW image rows below the last image row, of which the tensor itself holds Hs - kRefPad - H >= kRefPad; a group
// whose columns run past Ws wraps into the next row (+1).  The per-layer kernels over-read < 4096 slots.
constexpr int kRefSlackRows = kStreamRowsBelow - kRefPad + 1;
// Slots IN FRONT of a tensor (zero, never written): a strip's first group starts ROWS_ABOVE image rows above row 0
// (16 at dilation 8) and up to 2 DIL columns left of column 0, where the tensor's own border is kRefPad rows / columns
// (a column underrun wraps into the previous row: +1).  An fp16 activation tensor is allocated as
// [front | tensor | slack] and handed around by the address of `tensor`.
constexpr int kRefFrontRows = (kStreamRowsAbove > kRefPad ? kStreamRowsAbove - kRefPad : 0) + 1;
static_assert(kRefSlackRows == 24 && kRefFrontRows == 9, "zero rows around the fp16 tower tensors follow the StreamTile list");
size_t ref_slack(const RefGeom& g) {
  const size_t rows = (size_t)kRefSlackRows * g.Ws;
  return rows > 4096 ? rows : 4096;
}
size_t ref_front(const RefGeom& g) { return (size_t)kRefFrontRows * g.Ws; }
hipError_t alloc_ref16(const RefGeom& g, size_t tensor_and_slack_slots, uint4** raw, uint4** base) {
  const size_t front = ref_front(g), all = front + tensor_and_slack_slots;
  hipError_t e = dalloc(raw, all);
  if (e != hipSuccess) return e;
  e = memset_now(*raw, 0, all * sizeof(uint4));        // the zero borders are never written again
  *base = *raw + front;
  return e;
}

template <int DIL, int TW, int NBUF>
hipError_t launch_ref_f16x3(hipStream_t st, const RefLayerF16& L, const RefGeom& g, int num_cu, const uint4* in,
                            uint4* out, const uint4* res, size_t lo_slots, int nimg, bool lrelu, LaunchInfo* li = nullptr) {
  using T = RefTile2<DIL, TW>;
  constexpr int lds_bytes = NBUF * 2 * T::BUF * 16;
  auto kern = res ? k_ref_conv_f16x3<DIL, TW, NBUF, true> : k_ref_conv_f16x3<DIL, TW, NBUF, false>;
  hipError_t e = ensure_lds_attr(kern, lds_bytes);
  if (e != hipSuccess) return e;
  RefGeom gt = g;
  gt.tiles_x = (g.W + TW - 1) / TW;
  const int total = gt.tiles_x * gt.tiles_y * nimg;
  const int band = (total + 7) / 8;
  int cap = num_cu / 8;                      // one workgroup per CU (two on 8 x 32 tiles measured -6 %: the kernel is
                                             // memory bound and spills at 256 registers, profiles/r06_x3_wpc_ab.txt)
  if (cap < 1) cap = 1;
  const int rounds = (band + cap - 1) / cap;
  const int nlb = (band + rounds - 1) / rounds;
  report(li, nlb * 8, total);
  hipLaunchKernelGGL(kern, dim3(nlb * 8), dim3(256), lds_bytes, st, in, out, res, lo_slots, L.wfrag, L.bias, gt, nimg,
                     lrelu ? 1 : 0);
  return hipGetLastError();
}

hipError_t ref_conv_f16x3(hipStream_t st, const RefLayerF16& L, const RefGeom& g, int num_cu, int dil, const uint4* in,
                          uint4* out, const uint4* res, size_t lo_slots, int nimg, bool lrelu, LaunchInfo* li = nullptr) {
  switch (dil) {
    case 1: return launch_ref_f16x3<1, 64, 3>(st, L, g, num_cu, in, out, res, lo_slots, nimg, lrelu, li);
    case 2: return launch_ref_f16x3<2, 64, 3>(st, L, g, num_cu, in, out, res, lo_slots, nimg, lrelu, li);
    case 4: return launch_ref_f16x3<4, 32, 3>(st, L, g, num_cu, in, out, res, lo_slots, nimg, lrelu, li);
    case 8: return launch_ref_f16x3<8, 32, 2>(st, L, g, num_cu, in, out, res, lo_slots, nimg, lrelu, li);
    default: return hipErrorInvalidValue;
  }
}

template <int DIL, int TW, int NB = 3>
hipError_t launch_ref_f16_v2(hipStream_t st, const RefLayerF16& L, const RefGeom& g, int num_cu, const uint4* in,
                             uint4* out, const uint4* res, int nimg, bool lrelu, unsigned* tile_ctr, LaunchInfo* li = nullptr) {
  using T = RefTile2<DIL, TW, 8, NB>;
  // tile_ctr: the launch's tile queue (8 zeroed counters, 64 B apart)
  auto kern = res ? k_ref_conv_f16_v2<DIL, TW, true, 8, 2, NB> : k_ref_conv_f16_v2<DIL, TW, false, 8, 2, NB>;
  if (tile_ctr == nullptr) return hipErrorInvalidValue;
  if (T::LDS_BYTES > 64 * 1024) {
    hipError_t e = ensure_lds_attr(kern, T::LDS_BYTES);
    if (e != hipSuccess) return e;
  }
  static_assert(2 * T::LDS_BYTES <= 160 * 1024, "two tower workgroups per CU");
  RefGeom gt = g;                      // tile grid of this variant (the buffer geometry is for 8x64 tiles)
  gt.tiles_x = (g.W + TW - 1) / TW;
  gt.tiles_y = (g.H + 7) / 8;
  const int total = gt.tiles_x * gt.tiles_y * nimg;
  // persistent grid: 8 XCD bands, two workgroups per CU, every slot filled (the queue balances the bands)
  const int band = (total + 7) / 8;
  int cap = num_cu * 2 / 8;
  if (cap < 1) cap = 1;
  const int nlb = cap < band ? cap : band;
  report(li, nlb * 8, total);
  hipLaunchKernelGGL(kern, dim3(nlb * 8), dim3(256), T::LDS_BYTES, st, in, out, res, L.wfrag, L.bias, gt, nimg,
                     lrelu ? 1 : 0, tile_ctr);
  return hipGetLastError();
}

// Fused residual block, row-streaming form (sn_stream_block.hpp): one 512-thread workgroup per CU walks its share of
// the flattened (image, row phase, strip, sub-row) sequence.  x and y must be different tensors.  dump: >= 1 KB scratch.
template <class T>
hipError_t launch_ref_block_stream(hipStream_t st, const RefLayerF16& L1, const RefLayerF16& L2, const RefGeom& g, int num_cu,
                                   const uint4* x, uint4* y, int nimg, unsigned* dump, const HeadArgs& ha = HeadArgs{},
                                   LaunchInfo* li = nullptr) {
  constexpr int DIL = T::DIL;
  auto kern = k_ref_block_stream_f16<T::DIL, T::TW, T::R, T::NXS, T::NWR, T::HEAD>;
  if (dump == nullptr) return hipErrorInvalidValue;
  hipError_t e = ensure_lds_attr(kern, T::LDS_BYTES);
  if (e != hipSuccess) return e;
  StreamSched sc;
  // the tail form walks the OUTPUT maps (H x W of the head, <= the tensor's valid area), the others the whole tensor
  const int Wn = T::HEAD ? ha.W : g.W, Hn = T::HEAD ? ha.H : g.H;
  if (T::HEAD && (!ha.w || !ha.disp_low || (!ha.out_disp && !ha.out_raw) || ha.W > g.W || ha.H > g.H || ha.ups.rs > 0.5f)) return hipErrorInvalidValue;
  sc.nstrips = (Wn + T::OW - 1) / T::OW;
  sc.hsub = (Hn + DIL - 1) / DIL;
  sc.total_rows = nimg * DIL * sc.nstrips * sc.hsub;
  const int wg_env = switches().stream_wgs;     // experiment switch
  int nwg = wg_env > 0 ? wg_env : num_cu;
  if (nwg > sc.total_rows) nwg = sc.total_rows;
  if (nwg < 1) nwg = 1;
  sc.rows_per_wg = (sc.total_rows + nwg - 1) / nwg;
  const int grid = (sc.total_rows + sc.rows_per_wg - 1) / sc.rows_per_wg;
  report(li, grid, sc.total_rows);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), T::LDS_BYTES, st, x, y, L1.wfrag, L1.bias, L2.wfrag, L2.bias, g, sc,
                     reinterpret_cast<uint4*>(dump), ha);
  return hipGetLastError();
}

// Last block of the tower + the refinement head in one launch (tail form): y never leaves the CU, the head's maps are the
// only thing written.  Same arithmetic as the streamed block followed by k_head_final_f16 (bit-identical maps).
hipError_t ref_block_stream_tail(hipStream_t st, const RefLayerF16& L1, const RefLayerF16& L2, const RefGeom& g, int num_cu,
                                 const uint4* x, int nimg, unsigned* dump, const HeadArgs& ha, LaunchInfo* li = nullptr) {
  return launch_ref_block_stream<StreamTileTail>(st, L1, L2, g, num_cu, x, nullptr, nimg, dump, ha, li);
}

// Strip shapes: 64 columns x 4 rows per step for dilation 1 / 2 (62 / 60 of 64 columns are outputs); 128 columns x 2 rows
// for dilation 4 / 8, where a 64-wide strip would keep only 56 / 48 of its columns (120 / 112 of 128 here).
hipError_t ref_block_stream(hipStream_t st, const RefLayerF16& L1, const RefLayerF16& L2, const RefGeom& g, int num_cu, int dil,
                            const uint4* x, uint4* y, int nimg, unsigned* dump, LaunchInfo* li = nullptr) {
  switch (dil) {
    case 1: return launch_ref_block_stream<StreamTile1>(st, L1, L2, g, num_cu, x, y, nimg, dump, HeadArgs{}, li);
    case 2: return launch_ref_block_stream<StreamTile2>(st, L1, L2, g, num_cu, x, y, nimg, dump, HeadArgs{}, li);
    case 4: return launch_ref_block_stream<StreamTile4>(st, L1, L2, g, num_cu, x, y, nimg, dump, HeadArgs{}, li);
    case 8: return launch_ref_block_stream<StreamTile8>(st, L1, L2, g, num_cu, x, y, nimg, dump, HeadArgs{}, li);
    default: return hipErrorInvalidValue;
  }
}
// SN_STREAM_DIL: largest dilation that runs through the streaming kernel (default 8 = every block; 2 = round-3a behaviour)
inline bool stream_block_supports(int dil) {
  return (dil == 1 || dil == 2 || dil == 4 || dil == 8) && dil <= switches().stream_dil;
}

// k_head_final_f16 on the tower's output tensor x (split: hi + lo tensor, lo_slots behind it) for nimg maps
hipError_t launch_head_final_f16(hipStream_t st, bool split, const uint4* x, size_t lo_slots, const RefGeom& g, int nimg,
                                 const HeadArgs& ha) {
  constexpr int TH = 16;
  using T = HeadTile<TH>;
  const int tiles_x = (ha.W + T::TWO - 1) / T::TWO, tiles_y = (ha.H + TH - 1) / TH;
  const dim3 grid((unsigned)(tiles_x * tiles_y * nimg));
  if (split)
    hipLaunchKernelGGL((k_head_final_f16<true, TH>), grid, dim3(256), T::LDS_BYTES, st, x, lo_slots, g, tiles_x, tiles_y, ha);
  else
    hipLaunchKernelGGL((k_head_final_f16<false, TH>), grid, dim3(256), T::LDS_BYTES, st, x, (size_t)0, g, tiles_x, tiles_y, ha);
  return hipGetLastError();
}

// The SN_PREC_FP32 head on x fp32 [nimg][32][Hk][Wk]: the fp32 MFMA with the nine taps as M (k_head_final_mfma32), or the
// per-pixel kernel (SN_HEAD_MFMA32=0, A/B).  Geometry-free: refine_level and the parity hook sn_dbg_head both launch through it.
hipError_t launch_head_final_f32(hipStream_t st, bool mfma32, const float* x, int Hk, int Wk, int nimg, const HeadArgs& ha) {
  if (mfma32) {
    constexpr int TH = 14;               // 16-row P window: 32 segments, 8 per wave (TH = 6 measured the same 41 us without the statistic)
    using HT = HeadTile<TH>;
    const int tiles_x = (ha.W + HT::TWO - 1) / HT::TWO, tiles_y = (ha.H + TH - 1) / TH;
    hipLaunchKernelGGL(k_head_final_mfma32<TH>, dim3((unsigned)(tiles_x * tiles_y * nimg)), dim3(256), HT::LDS_BYTES, st, x,
                       Hk, Wk, tiles_x, tiles_y, ha);
  } else {
    dim3 grid((ha.W + 63) / 64, (ha.H + 3) / 4, nimg);
    hipLaunchKernelGGL(k_head_final, grid, dim3(256), 0, st, x, Hk, Wk, ha);
  }
  return hipGetLastError();
}

// The cost volume of m pairs from feat fp32 [2m][32][hl][wl], in split slots: the plain layout, or the zero-bordered one
hipError_t launch_cost_slots(hipStream_t st, const float* feat, uint4* vol, int Dl, int hl, int wl, int m) {
  const long total = (long)m * Dl * 4 * hl * wl;
  hipLaunchKernelGGL(k_cost_slots, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, feat, vol, Dl, hl, wl, m);
  return hipGetLastError();
}
hipError_t launch_cost_slots_pad(hipStream_t st, const float* feat, uint4* volp, const VolPad& g, int m) {
  const long total = (long)m * g.Dl * 4 * g.H * g.W;
  hipLaunchKernelGGL(k_cost_slots_pad, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, feat, volp, g, m);
  return hipGetLastError();
}

// One level of the hierarchical refinement's image pyramid for nimg images: 2x2 average pooling of the left eye into
// out [nimg][3][Ho][Wo].  first: src = the int8 model input [nimg][6][H][W]; otherwise the float level above (H, W unused).
hipError_t launch_img_pool2(hipStream_t st, bool first, const void* src, int H, int W, int Ho, int Wo, float* out, int nimg) {
  const long total = (long)nimg * 3 * Ho * Wo;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (first)
    hipLaunchKernelGGL(k_img_pool2<true>, grid, dim3(256), 0, st, src, H, W, Ho, Wo, out, total);
  else
    hipLaunchKernelGGL(k_img_pool2<false>, grid, dim3(256), 0, st, src, 0, 0, Ho, Wo, out, total);
  return hipGetLastError();
}

// Tile width of a dilation-1 / -2 launch.  The persistent grid (two workgroups per CU) works through the tiles in
// rounds and the launch lasts ceil(tiles / workgroups) rounds: 1280x720, two pairs = 3600 8x64 tiles on 512
// workgroups = 7.03 -> 8 rounds, 12 % of the launch spent on 16 leftover tiles.  8x32 tiles cost ~3 % more per pixel
// (per-tile waits and barriers, 34/32 instead of 66/64 halo columns) but quantise twice as finely (14.06 -> 15
// half-rounds = 7.5): measured +1.7 % end to end at 1280x720, +0.7 % at 1248x384.  Chosen per launch from the
// tile count; force_tw (parity hooks): 64 or 32.
inline int tower_tile_width(const RefGeom& g, int nimg, int num_cu, int force_tw) {
  if (force_tw == 32 || force_tw == 64) return force_tw;
  const long wgs = 2L * num_cu;
  const long rows = (g.H + 7) / 8;
  const long r64 = ((long)((g.W + 63) / 64) * rows * nimg + wgs - 1) / wgs;
  const long r32 = ((long)((g.W + 31) / 32) * rows * nimg + wgs - 1) / wgs;
  return (double)r32 * 0.5 * 1.03 < (double)r64 ? 32 : 64;
}

hipError_t ref_conv_f16(hipStream_t st, const RefLayerF16& L, const RefGeom& g, int num_cu, int dil, const uint4* in,
                        uint4* out, const uint4* res, int nimg, bool lrelu, unsigned* tile_ctr, int force_tw = 0,
                        LaunchInfo* li = nullptr) {
  if (dil <= 2 && tower_tile_width(g, nimg, num_cu, force_tw) == 32) {
    if (dil == 1) return launch_ref_f16_v2<1, 32>(st, L, g, num_cu, in, out, res, nimg, lrelu, tile_ctr, li);
    if (dil == 2) return launch_ref_f16_v2<2, 32>(st, L, g, num_cu, in, out, res, nimg, lrelu, tile_ctr, li);
  }
  switch (dil) {
    case 1: return launch_ref_f16_v2<1, 64>(st, L, g, num_cu, in, out, res, nimg, lrelu, tile_ctr, li);
    case 2: return launch_ref_f16_v2<2, 64>(st, L, g, num_cu, in, out, res, nimg, lrelu, tile_ctr, li);
    case 4: return launch_ref_f16_v2<4, 32>(st, L, g, num_cu, in, out, res, nimg, lrelu, tile_ctr, li);      // 61 KB ring
    case 8: return launch_ref_f16_v2<8, 32, 2>(st, L, g, num_cu, in, out, res, nimg, lrelu, tile_ctr, li);   // 74 KB, two buffers
    default: return hipErrorInvalidValue;
  }
}

// One residual block of the fp16 tower on `*cur` (input and, on return, output); `*oth` is scratch.  tile_ctr: the
// block's two tile queues (kTileCtrStride apart).
hipError_t ref_block_f16(hipStream_t st, const RefLayerF16& L1, const RefLayerF16& L2, const RefGeom& g, int num_cu,
                         int dil, uint4** cur, uint4** oth, int nimg, unsigned* tile_ctr, int fuse_mode, unsigned* dump,
                         bool alt = false, LaunchInfo* li = nullptr) {
  hipError_t e = hipErrorInvalidValue;
  bool fused = false;
  if (fuse_mode == 4 && stream_block_supports(dil)) {
    e = ref_block_stream(st, L1, L2, g, num_cu, dil, *cur, *oth, nimg, dump, li);
    fused = true;
  }
  if (fused) {
    uint4* t = *cur;
    *cur = *oth;
    *oth = t;
    return e;
  }
  e = ref_conv_f16(st, L1, g, num_cu, dil, *cur, *oth, nullptr, nimg, true, tile_ctr);
  if (e != hipSuccess) return e;
  RefGeom g2 = g;
  if (alt) g2.rev ^= 1;                  // the second conv walks the tiles the other way round (refine_level)
  return ref_conv_f16(st, L2, g2, num_cu, dil, *oth, *cur, *cur, nimg, true, tile_ctr + kTileCtrStride, 0, li);   // in-place residual
}

// Fused residual block on split operands, row-streaming form (sn_stream_block_x3.hpp): every dilation.  x and y are
// different hi tensors, the lo tensors sit lo_slots behind them.  SN_X3_STREAM=0 keeps two k_ref_conv_f16x3 launches (A/B).
inline bool stream_x3_supports(int dil) {
  return switches().x3_stream && (dil == 1 || dil == 2 || dil == 4 || dil == 8);
}
template <int DIL, int NWR = 2>
hipError_t launch_ref_block_stream_x3(hipStream_t st, const RefLayerF16& L1, const RefLayerF16& L2, const RefGeom& g, int num_cu,
                                      const uint4* x, uint4* y, size_t lo_slots, int nimg, LaunchInfo* li = nullptr) {
  using T = StreamTileX3<DIL, 64, 2, 5, NWR>;
  static_assert(T::ROWS_ABOVE <= kStreamRowsAbove && T::ROWS_BELOW <= kStreamRowsBelow, "inside the zero rows the tensors are allocated with");
  auto kern = k_ref_block_stream_x3<T::DIL, T::TW, T::R, T::NXS, T::NWR>;
  hipError_t e = ensure_lds_attr(kern, T::LDS_BYTES);
  if (e != hipSuccess) return e;
  StreamSched sc;
  sc.nstrips = (g.W + T::OW - 1) / T::OW;
  sc.hsub = (g.H + DIL - 1) / DIL;
  sc.total_rows = nimg * DIL * sc.nstrips * sc.hsub;
  int nwg = num_cu;
  if (nwg > sc.total_rows) nwg = sc.total_rows;
  if (nwg < 1) nwg = 1;
  sc.rows_per_wg = (sc.total_rows + nwg - 1) / nwg;
  const int grid = (sc.total_rows + sc.rows_per_wg - 1) / sc.rows_per_wg;
  report(li, grid, sc.total_rows);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(128 * T::NWR), T::LDS_BYTES, st, x, y, lo_slots * 16, L1.wfrag, L1.bias, L2.wfrag,
                     L2.bias, g, sc);
  return hipGetLastError();
}
// One residual block of the split tower on `*cur` (input and, on return, output); `*oth` is scratch.
hipError_t ref_block_f16x3(hipStream_t st, const RefLayerF16& L1, const RefLayerF16& L2, const RefGeom& g, int num_cu, int dil,
                           uint4** cur, uint4** oth, size_t lo_slots, int nimg, bool stream = true, LaunchInfo* li = nullptr) {
  if (stream && stream_x3_supports(dil)) {
    hipError_t e = hipErrorInvalidValue;
    // waves per role: 4 (default) = two waves per SIMD, one of each role, so that one role's epilogue / DMA issue sits beside the
    // other's MFMAs (256 registers per wave: 20 bytes of scratch at dilation 1 / 2); SN_X3_NWR=2 = one wave per SIMD (A/B)
    const int nwr = switches().x3_nwr;
    if (nwr == 4) {
      if (dil == 1) e = launch_ref_block_stream_x3<1, 4>(st, L1, L2, g, num_cu, *cur, *oth, lo_slots, nimg, li);
      else if (dil == 2) e = launch_ref_block_stream_x3<2, 4>(st, L1, L2, g, num_cu, *cur, *oth, lo_slots, nimg, li);
      else if (dil == 4) e = launch_ref_block_stream_x3<4, 4>(st, L1, L2, g, num_cu, *cur, *oth, lo_slots, nimg, li);
      else e = launch_ref_block_stream_x3<8, 4>(st, L1, L2, g, num_cu, *cur, *oth, lo_slots, nimg, li);
    } else if (dil == 1) e = launch_ref_block_stream_x3<1>(st, L1, L2, g, num_cu, *cur, *oth, lo_slots, nimg, li);
    else if (dil == 2) e = launch_ref_block_stream_x3<2>(st, L1, L2, g, num_cu, *cur, *oth, lo_slots, nimg, li);
    else if (dil == 4) e = launch_ref_block_stream_x3<4>(st, L1, L2, g, num_cu, *cur, *oth, lo_slots, nimg, li);
    else e = launch_ref_block_stream_x3<8>(st, L1, L2, g, num_cu, *cur, *oth, lo_slots, nimg, li);
    uint4* t = *cur;
    *cur = *oth;
    *oth = t;
    return e;
  }
  hipError_t e = ref_conv_f16x3(st, L1, g, num_cu, dil, *cur, *oth, nullptr, lo_slots, nimg, true);
  if (e != hipSuccess) return e;
  return ref_conv_f16x3(st, L2, g, num_cu, dil, *oth, *cur, *cur, lo_slots, nimg, true, li);      // in-place residual
}

}  // namespace
