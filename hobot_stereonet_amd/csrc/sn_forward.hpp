// sn_forward.hpp — the forward pass on device buffers: workspace allocation (alloc_ws / free_ws), the low-resolution
// branch, the refinement levels and their stream choreography (forward), stage profiling, the refinement statistic and
// the SN_PREC_AUTO controller with its repeat logic (run_forward).  Part of the single translation unit stereonet_hip.hip.
#pragma once

namespace {

// ---- workspace -----------------------------------------------------------------------------------
// Pairs per low-resolution piece and per tower launch of level k for a workspace of nb pairs with rb pairs per
// full-resolution launch: ONE definition shared by alloc_ws (buffer sizes) and sn_create's 32-bit offset guard.
inline int piece_pairs(const sn_handle* h, int nb, int rb) {
  int pb = h->piece > 0 ? h->piece : 16;
  if (pb > nb) pb = nb;
  if (pb < rb) pb = rb;
  return pb;
}
inline int level_chunk_pairs(int rb, int pb, int lv) {     // coarse level lv runs rb * 4^lv pairs per launch, at most a piece
  const long r = (long)rb << (2 * lv);
  return lv == 0 ? rb : (r < pb ? (int)r : pb);
}

// rb_x3: pairs per tower launch while an SN_PREC_AUTO handle runs in SN_PREC_F16X3 (0 = rb: every other precision)
int alloc_ws(sn_handle* h, Workspace* ws, int nb, int rb, int ns, int rb_x3 = 0) {
  const bool is_auto = h->precision == SN_PREC_AUTO;
  if (rb_x3 <= 0 || rb_x3 > rb) rb_x3 = rb;
  ws->nb = nb;
  ws->rb = rb;
  ws->rb_x3 = rb_x3;
  ws->ns = (ns > 1 && nb > rb) ? (ns < kMaxTowerStreams ? ns : kMaxTowerStreams) : 1;
  if (h->levels > 1) ws->ns = 1;      // the level maps of a piece live in one buffer set: one tower stream
  ws->pb = piece_pairs(h, nb, rb);
  const int pb = ws->pb;
  const size_t HW = (size_t)h->H * h->W, HWp = (size_t)h->Hp * h->Wp, hw = (size_t)h->hl * h->wl;
  HIP_TRY(h, dalloc(&ws->in6, (size_t)nb * 6 * HW));
  // fp16 modes keep the tensors between the down-convs in the zero-bordered layout (downp[], below) unless SN_DOWN_DMA=0
  // or a tensor would not fit 32-bit byte offsets; the plain ones are then not allocated at all (0.9 GB per 16-pair piece)
  bool padded_down = h->precision != SN_PREC_FP32 && switches().down_dma;
  size_t downp_bytes[3] = {0, 0, 0};
  // (folded down-convs 0 + 1: the half-resolution tensor never exists, so its size cannot veto the zero-bordered layout)
  for (int k = h->fold_down01 ? 1 : 0; k < 3 && padded_down; ++k) {      // input of down-conv k + 1: output grid (Hp, Wp) >> (k + 2)
    const SlotGeom g = down_in_geom(h->Hp >> (k + 2), h->Wp >> (k + 2));
    downp_bytes[k] = (size_t)2 * pb * 8 * g.PH * g.PW * sizeof(uint4);
    padded_down = downp_bytes[k] < ((size_t)1 << 32);
  }
  const int k_first = h->fold_down01 ? 1 : 0;       // folded down-convs 0 + 1: the half-resolution tensor never exists
  for (int k = k_first; k < 3 && !padded_down; ++k)
    HIP_TRY(h, dalloc(&ws->down[k], (size_t)2 * pb * kC * (HWp >> (2 * (k + 1)))));
  for (int k = 0; k < 3; ++k) HIP_TRY(h, dalloc(&ws->low[k], (size_t)2 * pb * kC * hw));
  HIP_TRY(h, dalloc(&ws->feat, (size_t)2 * pb * kC * hw));
  for (int k = 0; k < 2; ++k) HIP_TRY(h, dalloc(&ws->vol[k], (size_t)pb * h->Dl * kC * hw));
  for (int k = k_first; k < 3 && padded_down; ++k) {
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&ws->downp[k]), downp_bytes[k]));
    HIP_TRY(h, memset_now(ws->downp[k], 0, downp_bytes[k]));   // the borders stay zero: kernels write image pixels only
  }
  if (padded_down && switches().feat_dma) {       // (the last down-conv writes straight into the bordered layout)
    const FeatPad g = feat_pad(h->hl, h->wl);
    const size_t bytes = (size_t)2 * pb * g.img_slots() * sizeof(uint4);
    for (int k = 0; k < 2 && bytes < ((size_t)1 << 32); ++k) {
      HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&ws->lowp[k]), bytes));
      HIP_TRY(h, memset_now(ws->lowp[k], 0, bytes));       // the borders stay zero: kernels write image pixels only
    }
  }
  if (h->precision != SN_PREC_FP32 && switches().agg_dma) {
    const VolPad g = vol_pad(h->Dl, h->hl, h->wl);
    const size_t bytes = g.planes(pb) * g.plane_slots() * sizeof(uint4);
    // the kernel addresses the volume with 32-bit byte offsets; a piece that large keeps the plain volumes
    for (int k = 0; k < 2 && bytes < ((size_t)1 << 32); ++k) {
      HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&ws->volp[k]), bytes));
      HIP_TRY(h, memset_now(ws->volp[k], 0, bytes));       // the borders stay zero: kernels write image pixels only
    }
  }
  HIP_TRY(h, dalloc(&ws->cost, (size_t)nb * h->Dl * hw));
  HIP_TRY(h, dalloc(&ws->disp_low, (size_t)nb * hw));
  HIP_TRY(h, dalloc(&ws->conf_low, (size_t)nb * hw));
  HIP_TRY(h, memset_now(ws->conf_low, 0, (size_t)nb * hw * sizeof(float)));      // sn_dbg_read("conf_low") before any sn_infer_conf: zeros
  // hi tensor (+ lo tensor behind it in SN_PREC_F16X3).  An AUTO handle keeps the fp16 layout for rb pairs and puts the lo
  // tensor of its (smaller) split chunks BEHIND that region: the split mode's hi tensor then sits where the fp16 tensors of
  // the first pairs do — same image pixels, same zero borders — and the lo tensor never touches a border of the fp16
  // layout (with the lo tensor directly behind rb_x3 pairs its pixels landed on the zero borders of pair rb_x3's fp16 plane:
  // the first fp16 call after a split call then read non-zero padding — caught by tests/test_gpu_auto.py)
  auto tensor_slots = [&](const RefGeom& rg, int pairs, int pairs_x3) {
    const size_t one = ref16_slots(rg, pairs) + ref_slack(rg), lo = ref16_slots(rg, pairs_x3) + ref_slack(rg);
    return h->precision == SN_PREC_F16X3 ? 2 * one : (is_auto ? one + lo : one);
  };
  if (h->precision == SN_PREC_FP32) {
    for (int k = 0; k < 2 * ws->ns; ++k) HIP_TRY(h, dalloc(&ws->ref[k], (size_t)rb * kC * HWp));
  } else {
    for (int k = 0; k < 2 * ws->ns; ++k)
      HIP_TRY(h, alloc_ref16(h->tw[0].rg, tensor_slots(h->tw[0].rg, rb, rb_x3), &ws->ref16_raw[k], &ws->ref16[k]));
    // fine-grained: the queue words must be coherent across the 8 XCD L2s at device scope and with the memset
    // one counter block per tower chunk of a forward(): chunks never straddle a low-resolution piece, so every
    // piece may end with one short chunk (forward() numbers the chunks with a running ordinal)
    // a hierarchical model adds the coarse-level launches of every piece: one block per (piece, level, coarse chunk)
    ws->n_chunks = (nb + rb_x3 - 1) / rb_x3 + (nb + pb - 1) / pb + 2;
    for (int lv = 1; lv < h->levels; ++lv) {
      const int rbk = level_chunk_pairs(rb_x3, pb, lv);
      ws->n_chunks += ((nb + pb - 1) / pb + 2) * ((pb + rbk - 1) / rbk + 1);
    }
    HIP_TRY(h, hipExtMallocWithFlags(reinterpret_cast<void**>(&ws->tile_ctr), kTileCtrBytes * ws->n_chunks, hipDeviceMallocFinegrained));
  }
  ws->rbk[0] = rb;
  ws->rbk_x3[0] = rb_x3;
  for (int lv = 1; lv < h->levels; ++lv) {
    const Tower& T = h->tw[lv];
    const size_t HWk = (size_t)T.Hk * T.Wk;
    ws->rbk[lv] = level_chunk_pairs(rb, pb, lv);
    ws->rbk_x3[lv] = level_chunk_pairs(rb_x3, pb, lv);
    for (int k = 0; k < 2; ++k) {
      if (h->precision == SN_PREC_FP32) {
        HIP_TRY(h, dalloc(&ws->ref_lv[lv][k], (size_t)ws->rbk[lv] * kC * HWk));
      } else {
        HIP_TRY(h, alloc_ref16(T.rg, tensor_slots(T.rg, ws->rbk[lv], ws->rbk_x3[lv]), &ws->ref16_lv_raw[lv][k], &ws->ref16_lv[lv][k]));
      }
    }
    HIP_TRY(h, dalloc(&ws->pyr[lv], (size_t)pb * 3 * HWk));
    HIP_TRY(h, dalloc(&ws->lvl_disp[lv], (size_t)pb * HWk));
  }
  HIP_TRY(h, dalloc(&ws->out_disp, (size_t)nb * HW));
  HIP_TRY(h, dalloc(&ws->out_raw, (size_t)nb * HW));
  HIP_TRY(h, dalloc(&ws->nv12, (size_t)HW * 3));
  HIP_TRY(h, dalloc(&ws->stats, kStatU64));
  HIP_TRY(h, memset_now(ws->stats, 0, kStatU64 * sizeof(unsigned long long)));
  HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&ws->stats_host), kStatU64 * sizeof(unsigned long long), hipHostMallocDefault));
  memset(ws->stats_host, 0, kStatU64 * sizeof(unsigned long long));
  return SN_OK;
}

void free_ws(Workspace* ws) {
  hipFree(ws->in6);
  hipFree(ws->tile_ctr);
  for (auto p : ws->down) hipFree(p);
  for (auto p : ws->low) hipFree(p);
  hipFree(ws->feat);
  for (auto p : ws->vol) hipFree(p);
  for (auto p : ws->volp) hipFree(p);
  for (auto p : ws->downp) hipFree(p);
  for (auto p : ws->lowp) hipFree(p);
  hipFree(ws->cost);
  hipFree(ws->disp_low);
  hipFree(ws->conf_low);
  for (auto p : ws->ref) hipFree(p);
  for (auto p : ws->ref16_raw) hipFree(p);
  for (auto& lv : ws->ref_lv)
    for (auto p : lv) hipFree(p);
  for (auto& lv : ws->ref16_lv_raw)
    for (auto p : lv) hipFree(p);
  for (auto p : ws->pyr) hipFree(p);
  for (auto p : ws->lvl_disp) hipFree(p);
  hipFree(ws->out_disp);
  hipFree(ws->out_raw);
  hipFree(ws->nv12);
  hipFree(ws->stats);
  if (ws->stats_host) hipHostFree(ws->stats_host);
  *ws = Workspace();
}

// ---- the forward pass on device buffers ------------------------------------------------------------
// The soft-argmin of npix = (pairs) hl wl pixels on caller buffers, every precision; the one place that names its kernels.
// folded: v holds the partial sums P of the last aggregation layer (k_softargmin_p; w unused), otherwise its volume, which
// k_head_softargmin contracts with w [32][27] first.  cost_out / conf_low nullable; nf: the range check's count (nullable).
hipError_t launch_softargmin_kernels(hipStream_t st, const float* v, bool folded, const float* w, float bias, int Dl, int hl,
                                     int wl, int npix, float* disp_low, float* cost_out, float* conf_low, unsigned long long* nf) {
  const bool want_conf = conf_low != nullptr;
  const dim3 grid((npix + 63) / 64);
  if (folded) {
    const auto kern = want_conf ? k_softargmin_p<16, true> : k_softargmin_p<16, false>;
    hipLaunchKernelGGL(kern, grid, dim3(64 * Dl), 0, st, v, bias, Dl, hl, wl, npix, disp_low, cost_out, conf_low, nf);
  } else {
    const auto kern = want_conf ? k_head_softargmin<16, true> : k_head_softargmin<16, false>;
    hipLaunchKernelGGL(kern, grid, dim3(64 * kSamWaves), 0, st, v, w, bias, Dl, hl, wl, npix, disp_low, cost_out, conf_low, nf);
  }
  return hipGetLastError();
}

// The soft-argmin of pairs [p0, p0 + m) on the workspace's buffers (launch_softargmin_kernels, above, names the kernels).  folded: v
// holds the partial sums P of the last aggregation layer (SN_HEAD_FOLD on the zero-bordered volumes), otherwise its volume.
// Writes disp_low, and cost / conf_low on request.
int launch_softargmin(sn_handle* h, Workspace& ws, hipStream_t st, const float* v, bool folded, int p0, int m, bool want_cost,
                      bool want_conf) {
  const int hl = h->hl, wl = h->wl, Dl = h->Dl, npix = m * hl * wl;
  float* const disp_low = ws.disp_low + (size_t)p0 * hl * wl;
  float* const cost_out = want_cost ? ws.cost + (size_t)p0 * Dl * hl * wl : nullptr;
  float* const conf_low = want_conf ? ws.conf_low + (size_t)p0 * hl * wl : nullptr;
  HIP_TRY(h, launch_softargmin_kernels(st, v, folded, h->aout.w, h->aout.bias, Dl, hl, wl, npix, disp_low, cost_out, conf_low,
                                       ws.stats + kStatNonfiniteLow));
  return SN_OK;
}

// Low-resolution branch of the fp16 modes on split-slot activations (SlotIn): every layer's epilogue writes the
// hi/lo fp16 pair its consumer's split-operand MFMAs read, the weights-stationary kernel stages them as plain
// 16-byte copies.  Only the tensors other kernels read stay fp32 NCHW: the feature map (cost-volume loader, parity
// hook) and the last aggregation volume (soft-argmin head).  Three stages; each runs on the zero-bordered layout and its
// LDS-DMA kernel where alloc_ws made the tensors, on the plain one otherwise.
inline const uint4* as_slots(const float* p) { return reinterpret_cast<const uint4*>(p); }

// down-convs: int8 input `in` of ni images -> ws.lowp[0] (zero-bordered feature layout) or ws.low[0]
int lowres_down_slots(sn_handle* h, Workspace& ws, hipStream_t st, const int8_t* in, int ni) {
  const int Hp = h->Hp, Wp = h->Wp, ncu = h->num_cu;
  const int k_first = h->fold_down01 ? 1 : 0;       // folded: down-convs 0 and 1 as one 13x13 stride-4 conv straight from the int8 input (sn_down01.hpp)
  if (ws.downp[1] != nullptr) {       // zero-bordered tensors between the down-convs, LDS-DMA kernel
    SlotGeom gin[3];
    for (int i = 0; i < 3; ++i) gin[i] = down_in_geom(Hp >> (i + 2), Wp >> (i + 2));
    if (h->fold_down01)
      HIP_TRY(h, launch_down01(st, h->down01, in, h->H, h->W, ni, Hp / 4, Wp / 4, ws.downp[1], gin[1], ncu));
    else
      HIP_TRY(h, launch_down0_f16(st, h->down0, h->down[0].bias, in, h->H, h->W, ni, Hp / 2, Wp / 2,
                                  reinterpret_cast<float*>(ws.downp[0]), ncu, &gin[0]));
    for (int i = k_first; i < 3; ++i) {
      const int Ho = Hp >> (i + 2), Wo = Wp >> (i + 2);
      const SlotGeom plain{Ho, Wo, 0, 0};
      const FeatPad fp = feat_pad(h->hl, h->wl);
      const SlotGeom bordered{fp.PH, fp.PW, 1, 1};           // the feature layers' zero-bordered layout (sn_feat_dma.hpp)
      void* const last = ws.lowp[0] ? (void*)ws.lowp[0] : (void*)ws.low[0];
      HIP_TRY(h, launch_down_dma(st, h->down[i + 1], ws.downp[i], ni, Ho, Wo, i < 2 ? (void*)ws.downp[i + 1] : last,
                                 i < 2 ? gin[i + 1] : (ws.lowp[0] ? bordered : plain), false, ncu));
    }
    return SN_OK;
  }
  if (h->fold_down01)
    HIP_TRY(h, launch_down01(st, h->down01, in, h->H, h->W, ni, Hp / 4, Wp / 4, reinterpret_cast<uint4*>(ws.down[1]),
                             SlotGeom{Hp / 4, Wp / 4, 0, 0}, ncu));
  else
    HIP_TRY(h, launch_down0_f16(st, h->down0, h->down[0].bias, in, h->H, h->W, ni, Hp / 2, Wp / 2, ws.down[0], ncu));
  float* const src[3] = {ws.down[0], ws.down[1], ws.down[2]};
  float* const dst[3] = {ws.down[1], ws.down[2], ws.low[0]};
  for (int i = k_first; i < 3; ++i) {
    const int Hi = Hp >> (i + 1), Wi = Wp >> (i + 1);
    if ((h->ablate_x >> (kAblDown + i)) & 1u) HIP_TRY(h, zero_lo_slots(st, src[i], ni, (size_t)Hi * Wi));
    SlotIn ld{as_slots(src[i]), 0, Hi, Wi};
    HIP_TRY(h, (launch_conv_x3s<5, 2, 32, 4, 32, 32, 1, true, SlotIn>(st, h->down[i + 1], ld, ni, Hi / 2, Wi / 2, dst[i],
                                                                     nullptr, false, ncu)));
  }
  return SN_OK;
}

// feature tower: six residual blocks + the output conv on ni images -> ws.feat (fp32 NCHW)
int lowres_features_slots(sn_handle* h, Workspace& ws, hipStream_t st, int ni) {
  const int hl = h->hl, wl = h->wl, ncu = h->num_cu;
  if (ws.lowp[0] != nullptr && ws.downp[1] != nullptr) {     // zero-bordered (x, t), LDS-DMA kernel
    const FeatPad fp = feat_pad(hl, wl);
    uint4 *x = ws.lowp[0], *t = ws.lowp[1];
    // (one launch per layer: a single launch for all twelve with per-image group barriers in device memory was built and
    // measured in round 5 — bit-identical, 609 us instead of 167 us per 16-pair piece: an agent-scope hand-off costs several
    // kernel boundaries, DESIGN.md §5d, profiles/r05_feat_chain_ab.txt)
    for (int i = 0; i < kNFeatRes; ++i) {
      HIP_TRY(h, (launch_feat_dma<true, false>(st, h->fres[i][0], x, fp, ni, t, nullptr, true, ncu)));
      HIP_TRY(h, (launch_feat_dma<true, true>(st, h->fres[i][1], t, fp, ni, x, x, true, ncu)));     // in-place residual
    }
    HIP_TRY(h, (launch_feat_dma<false, false>(st, h->fout, x, fp, ni, ws.feat, nullptr, false, ncu)));
    return SN_OK;
  }
  float *const x = ws.low[0], *const t = ws.low[1];
  const SlotIn lx{as_slots(x), 0, hl, wl}, lt{as_slots(t), 0, hl, wl};
  for (int i = 0; i < kNFeatRes; ++i) {
    if ((h->ablate_x >> (kAblFeat + 2 * i)) & 1u) HIP_TRY(h, zero_lo_slots(st, x, ni, (size_t)hl * wl));
    HIP_TRY(h, (launch_conv_x3s<3, 1, 32, 8, 16, 16, 2, true, SlotIn>(st, h->fres[i][0], lx, ni, hl, wl, t, nullptr, true, ncu)));
    if ((h->ablate_x >> (kAblFeat + 2 * i + 1)) & 1u) HIP_TRY(h, zero_lo_slots(st, t, ni, (size_t)hl * wl));
    HIP_TRY(h, (launch_conv_x3s<3, 1, 32, 8, 16, 16, 2, true, SlotIn>(st, h->fres[i][1], lt, ni, hl, wl, x, x, true, ncu)));
  }
  if ((h->ablate_x >> (kAblFeat + 12)) & 1u) HIP_TRY(h, zero_lo_slots(st, x, ni, (size_t)hl * wl));
  HIP_TRY(h, (launch_conv_x3s<3, 1, 32, 8, 16, 16, 1, false, SlotIn>(st, h->fout, lx, ni, hl, wl, ws.feat, nullptr, false, ncu)));
  return SN_OK;
}

// cost volume -> slots (vol[1]), then every aggregation layer reads slots: agg0 vol[1] -> vol[0], agg1 -> vol[1], ...; the
// last layer writes fp32 into ws.vol[(kNAgg - 1) & 1] either way.  *folded: what it wrote are the output conv's partial
// sums P [m Dl][27][hl][wl] (the contraction rides on the last layer's epilogue), not the volume.
int lowres_aggregate_slots(sn_handle* h, Workspace& ws, hipStream_t st, int m, bool* folded) {
  const int hl = h->hl, wl = h->wl, Dl = h->Dl, ncu = h->num_cu;
  *folded = false;
  if (ws.volp[0] != nullptr) {        // zero-bordered volumes, LDS-DMA kernel
    const VolPad g = vol_pad(Dl, hl, wl);
    HIP_TRY(h, launch_cost_slots_pad(st, ws.feat, ws.volp[1], g, m));
    for (int i = 0; i + 1 < kNAgg; ++i)
      HIP_TRY(h, launch_agg_dma<true>(st, h->agg[i], ws.volp[(i + 1) & 1], g, m, ws.volp[i & 1], true, ncu));
    const int i = kNAgg - 1;
    *folded = switches().head_fold && h->aout.pfrag;
    if (*folded)
      HIP_TRY(h, (launch_agg_dma<false, true>(st, h->agg[i], ws.volp[(i + 1) & 1], g, m, ws.vol[i & 1], true, ncu, h->aout.pfrag)));
    else
      HIP_TRY(h, launch_agg_dma<false>(st, h->agg[i], ws.volp[(i + 1) & 1], g, m, ws.vol[i & 1], true, ncu));
    return SN_OK;
  }
  HIP_TRY(h, launch_cost_slots(st, ws.feat, reinterpret_cast<uint4*>(ws.vol[1]), Dl, hl, wl, m));
  for (int i = 0; i < kNAgg; ++i) {
    float* const src = ws.vol[(i + 1) & 1];
    if ((h->ablate_x >> (kAblAgg + i)) & 1u) HIP_TRY(h, zero_lo_slots(st, src, m * Dl, (size_t)hl * wl));
    SlotIn lv{as_slots(src), Dl, hl, wl};
    if (i + 1 < kNAgg)
      HIP_TRY(h, (launch_conv_x3s<3, 1, 96, 8, 16, 16, 1, true, SlotIn>(st, h->agg[i], lv, m * Dl, hl, wl, ws.vol[i & 1], nullptr, true, ncu)));
    else
      HIP_TRY(h, (launch_conv_x3s<3, 1, 96, 8, 16, 16, 1, false, SlotIn>(st, h->agg[i], lv, m * Dl, hl, wl, ws.vol[i & 1], nullptr, true, ncu)));
  }
  return SN_OK;
}

// Low-resolution branch for pairs [p0, p0+m): Siamese features -> cost volume -> 3-D aggregation ->
// soft-argmin.  Intermediate buffers are piece-local; disp_low (and cost, conf_low) are indexed by p0.  want_conf: the
// soft-argmin epilogue also writes the confidence plane conf_low (sn_infer_conf).
int lowres(sn_handle* h, Workspace& ws, hipStream_t st, int p0, int m, const int8_t* in6, bool want_cost, bool want_conf,
           bool prof) {
  const int Hp = h->Hp, Wp = h->Wp, hl = h->hl, wl = h->wl, Dl = h->Dl;
  const size_t HW = (size_t)h->H * h->W;
  const int8_t* in = in6 + (size_t)p0 * 6 * HW;
  bool folded = false;
  if (h->precision != SN_PREC_FP32) {
    int rc;
    if ((rc = lowres_down_slots(h, ws, st, in, 2 * m))) return rc;
    if ((rc = lowres_features_slots(h, ws, st, 2 * m))) return rc;
    if (prof) HIP_TRY(h, hipEventRecord(h->ev[1], st));
    if ((rc = lowres_aggregate_slots(h, ws, st, m, &folded))) return rc;
    return launch_softargmin(h, ws, st, ws.vol[(kNAgg - 1) & 1], folded, p0, m, want_cost, want_conf);
  }
  // SN_PREC_FP32: every layer on the exact-fp32 MFMA, fp32 NCHW activations
  // --- Siamese feature tower: images = 2m (left, right interleaved), shared weights ---
  {
    LoadI8Eye ld{in, h->H, h->W};
    const int Ho = Hp / 2, Wo = Wp / 2;
    if (Ho * Wo <= 64 * 128)
      HIP_TRY(h, (launch_conv<5, 2, 1, 4, 4, 32>(st, h->down[0], ld, 2 * m, Ho, Wo, ws.down[0], nullptr, false)));
    else
      HIP_TRY(h, (launch_conv<5, 2, 1, 4, 8, 64>(st, h->down[0], ld, 2 * m, Ho, Wo, ws.down[0], nullptr, false)));
  }
  HIP_TRY(h, conv5x5s2(st, h->down[1], ws.down[0], 2 * m, Hp / 2, Wp / 2, ws.down[1]));
  HIP_TRY(h, conv5x5s2(st, h->down[2], ws.down[1], 2 * m, Hp / 4, Wp / 4, ws.down[2]));
  HIP_TRY(h, conv5x5s2(st, h->down[3], ws.down[2], 2 * m, Hp / 8, Wp / 8, ws.low[0]));
  float* x = ws.low[0];
  float* t = ws.low[1];
  for (int i = 0; i < kNFeatRes; ++i) {
    HIP_TRY(h, conv3x3(st, h->fres[i][0], x, 2 * m, hl, wl, 1, t, nullptr, true));
    HIP_TRY(h, conv3x3(st, h->fres[i][1], t, 2 * m, hl, wl, 1, x, x, true));   // in-place residual
  }
  HIP_TRY(h, conv3x3(st, h->fout, x, 2 * m, hl, wl, 1, ws.feat, nullptr, false));
  if (prof) HIP_TRY(h, hipEventRecord(h->ev[1], st));

  // --- cost volume (fused into the first 3-D conv's loader) + 3-D aggregation + soft-argmin ---
  LoadCostVol ld{ws.feat, Dl, hl, wl};
  HIP_TRY(h, (launch_conv<3, 1, 1, 8, 4, 32>(st, h->agg[0], ld, m * Dl, hl, wl, ws.vol[0], nullptr, true)));
  for (int i = 1; i < kNAgg; ++i) {
    LoadVol3D lv{ws.vol[(i - 1) & 1], Dl, hl, wl};
    HIP_TRY(h, (launch_conv<3, 1, 1, 8, 4, 32>(st, h->agg[i], lv, m * Dl, hl, wl, ws.vol[i & 1], nullptr, true)));
  }
  return launch_softargmin(h, ws, st, ws.vol[(kNAgg - 1) & 1], folded, p0, m, want_cost, want_conf);
}

// Pieces of one forward(): [p0, p0 + m), ws.pb pairs each.  Rounds 1-4 started with a short piece (2-4 pairs: the towers
// can only start when the first piece's low-resolution branch is done).  With the round-5 low-resolution branch a whole
// first piece measures faster in the fp16 modes (fewer, fuller launches of kernels that are mostly fixed cost: 3041-3049 ->
// 3064-3068 pairs/s at 1280x720, 4070 -> 4121 at 1242x375, profiles/r05_schedule_sweep.txt) — the device is never idle
// either way, so what counts is the sum of the kernel times.  SN_PREC_FP32 keeps the short first piece: its low-resolution
// branch (generic fp32 kernel) is five times longer.  SN_FIRST_PIECE=n forces n pairs.
inline int first_piece(const sn_handle* h, const Workspace& ws, int n) {
  const int forced = switches().first_piece;     // experiment switch
  int m = ws.pb;
  if (h->precision == SN_PREC_FP32) m = ws.rb * ws.ns > 2 ? ws.rb * ws.ns : 2;
  if (forced > 0) m = forced;
  if (m > ws.pb) m = ws.pb;
  return m < n ? m : n;
}

// One refinement level of one tower chunk: what refine_level runs, filled by refine_coarse and refine_chunk.
struct RefineCall {
  const Tower* T;             // the level's tower (weights + geometry)
  float* const* ref;          // its activation pair ref[0], ref[1]: fp32 ...
  uint4* const* ref16;        // ... or the fp16 modes
  const float* src;           // [c][sh][sw] map the level starts from
  int sh, sw;                 // its size
  UpScale ups;                // its upsample: x16 (the soft-argmin map, single-scale) or x2 (the level below, hierarchical)
  const void* img_src;        // int8 model input of the chunk (pyr = false) or the level's float image pyramid [c][3][Hk][Wk]
  bool pyr;
  int H, W;                   // size of the level's output map (the image for level 0, the whole padded level otherwise)
  float dnorm;                // D / 2^level: disparity normalisation at the tower input and residual scale at its output
  float* od;                  // float map and
  int32_t* orw;               // (level 0 only) wire map, both nullable
  unsigned* chunk_ctr;        // the chunk's tile-queue block (take_ctr_block)
  int c;                      // pairs of this chunk
  int cap;                    // pairs the hi region of the activation buffers holds: the lo tensor of SN_PREC_F16X3 starts behind it (c <= cap)
  bool pe;                    // record the profiling events of the tower
  int mode;                   // SN_PREC_F16 / SN_PREC_F16X3 / SN_PREC_FP32: the arithmetic of this call (an SN_PREC_AUTO handle holds two)
  unsigned long long* stat;   // the level's refinement statistic (sum of |D r|, refine_stat_commit)
};

int refine_level(sn_handle* h, Workspace& ws, hipStream_t st, const RefineCall& a) {
  const Tower& T = *a.T;
  const int ncu = h->num_cu, c = a.c;
  const int tcu = ws.tower_cu > 0 ? ws.tower_cu : ncu;      // workgroups of the streamed tower launches
  const int Hk = T.Hk, Wk = T.Wk;
  const bool pe = a.pe;
  // The wire factor is the reference's literal 16 * 12 for EVERY dmax (parser.cpp:86, stereonet_node.cpp:288,
  // publisher_member_function.py:75): the unmodified consumers recover pixels whatever D the model was built for.
  const float inv_q = (float)(1.0 / (kWireFactor * (double)kOutScale));
  if (a.mode == SN_PREC_FP32) {
    LoadRefineIn ld{a.src, reinterpret_cast<const int8_t*>(a.img_src), a.sh, a.sw, a.H, a.W, Hk, Wk, 1.0f / a.dnorm, a.ups,
                    a.pyr ? reinterpret_cast<const float*>(a.img_src) : nullptr};
    if (Hk * Wk <= 64 * 128)
      HIP_TRY(h, (launch_conv<3, 1, 1, 4, 4, 32>(st, T.rin, ld, c, Hk, Wk, a.ref[0], nullptr, true)));
    else
      HIP_TRY(h, (launch_conv<3, 1, 1, 4, 8, 64>(st, T.rin, ld, c, Hk, Wk, a.ref[0], nullptr, true)));
    if (pe) HIP_TRY(h, hipEventRecord(h->ev[4], st));
    for (int i = 0; i < kNRefRes; ++i) {
      HIP_TRY(h, conv3x3(st, T.rres[i][0], a.ref[0], c, Hk, Wk, kRefDil[i], a.ref[1], nullptr, true, ncu));
      HIP_TRY(h, conv3x3(st, T.rres[i][1], a.ref[1], c, Hk, Wk, kRefDil[i], a.ref[0], a.ref[0], true, ncu));
    }
    if (pe) HIP_TRY(h, hipEventRecord(h->ev[5], st));
    const HeadArgs ha{T.rout.w, a.src, a.od, a.orw, T.rout.bias, a.dnorm, inv_q, a.sh, a.sw, a.H, a.W, a.ups, a.stat};
    // head on the fp32 MFMA with the nine taps as M (k_head_final_mfma32); SN_HEAD_MFMA32=0 keeps the per-pixel kernel (A/B)
    HIP_TRY(h, launch_head_final_f32(st, switches().head_mfma32, a.ref[0], Hk, Wk, c, ha));
  } else {
    // fp16 tower: ref.in writes the NCHW8c fp16 tensor, the 12 C->C convs run on v_mfma_f32_32x32x16_f16, the head
    // reads fp16 and finishes in fp32
    uint4 *x16 = a.ref16[0], *t16 = a.ref16[1];
    if (pe) h->dom_pairs = 0;
    // Consecutive launches of a tower walk their tiles in OPPOSITE directions (g.rev): a launch then starts on the part
    // of the tensor its predecessor wrote LAST — what a cache that is slightly too small for the chunk still holds —
    // instead of on the lines an LRU policy has just evicted.
    // Neutral while the chunk fits the Infinity Cache (1280x720, two pairs: 2304 vs 2290 pairs/s), +11 % when it does
    // not (three pairs: 82 instead of 95 us per launch; any geometry whose single pair exceeds the cache).  SN_REV=0
    // disables it (diagnostic).
    const bool rev_env = switches().rev;
    RefGeom g = T.rg;
    int launch_no = 0;
    auto flip = [&]() { g.rev = rev_env ? (launch_no++ & 1) : 0; };
    flip();
    const bool x3 = a.mode == SN_PREC_F16X3;
    const size_t lo_slots = ref16_slots(g, a.cap) + ref_slack(g);         // hi tensor -> lo tensor (F16X3); cap = pairs the buffers hold
    HIP_TRY(h, launch_refin_f16(st, T.refin, T.rin.bias, a.src, a.img_src, a.pyr, a.sh, a.sw, a.H, a.W, 1.0f / a.dnorm, a.ups, g,
                                c, x16, x3, lo_slots * 16, ncu));
    if (pe) HIP_TRY(h, hipEventRecord(h->ev[4], st));
    flip();
    const HeadArgs ha{T.rout.wsplit, a.src, a.od, a.orw, T.rout.biassplit, a.dnorm * T.rout.unscale, inv_q, a.sh, a.sw,
                      a.H, a.W, a.ups, a.stat};
    // tail form: the streamed last block computes the head too (its output tensor is never written, no head launch)
    const bool last_streamed = h->fuse_mode == 4 && stream_block_supports(kRefDil[kNRefRes - 1]);
    const bool tail = !x3 && last_streamed && h->tail_fuse && kRefDil[kNRefRes - 1] == 1 && a.ups.rs <= 0.5f;
    for (int i = 0; i < kNRefRes; ++i) {
      if (x3) {
        const bool dom = pe && stream_x3_supports(kRefDil[i]) && h->dom_pairs < 6;
        if (dom) HIP_TRY(h, hipEventRecord(h->ev_dom[2 * h->dom_pairs], st));
        HIP_TRY(h, ref_block_f16x3(st, T.rres16x3[i][0], T.rres16x3[i][1], g, tcu, kRefDil[i], &x16, &t16, lo_slots, c));
        if (dom) HIP_TRY(h, hipEventRecord(h->ev_dom[2 * h->dom_pairs++ + 1], st));
      } else if (tail && i == kNRefRes - 1) {
        if (pe) HIP_TRY(h, hipEventRecord(h->ev[5], st));          // the plain tower launches end here
        HIP_TRY(h, ref_block_stream_tail(st, T.rres16[i][0], T.rres16[i][1], g, tcu, x16, c, h->dump, ha));
      } else {
        const bool dom = pe && h->fuse_mode == 4 && stream_block_supports(kRefDil[i]) && h->dom_pairs < 6;
        if (dom) HIP_TRY(h, hipEventRecord(h->ev_dom[2 * h->dom_pairs], st));
        HIP_TRY(h, ref_block_f16(st, T.rres16[i][0], T.rres16[i][1], g, tcu, kRefDil[i], &x16, &t16, c,
                                 a.chunk_ctr + 2 * i * kTileCtrStride, h->fuse_mode, h->dump, rev_env));
        if (dom) HIP_TRY(h, hipEventRecord(h->ev_dom[2 * h->dom_pairs++ + 1], st));
      }
    }
    if (!tail) {
      if (pe) HIP_TRY(h, hipEventRecord(h->ev[5], st));
      HIP_TRY(h, launch_head_final_f16(st, x3, x16, lo_slots, g, c, ha));
    }
  }
  HIP_TRY(h, hipGetLastError());
  return SN_OK;
}

// pairs per tower launch of level lv for a call in `mode` (an SN_PREC_AUTO handle in SN_PREC_F16X3 packs fewer pairs into the
// same buffers)
inline int chunk_pairs(const sn_handle* h, const Workspace& ws, int mode, int lv = 0) {
  return (h->precision == SN_PREC_AUTO && mode == SN_PREC_F16X3) ? ws.rbk_x3[lv] : ws.rbk[lv];
}

// Next tile-queue block of this forward() (nullptr for the fp32 path, which has no queues); the pool is sized by
// alloc_ws for the worst case, running past it would alias another launch's counters -> refuse loudly.
inline int take_ctr_block(sn_handle* h, Workspace& ws, int* ctr_block, unsigned** out) {
  *out = nullptr;
  if (!ws.tile_ctr) return SN_OK;
  if (*ctr_block >= ws.n_chunks) {
    set_err(h, "internal: tile-queue pool exhausted");
    return SN_ERR_DEVICE;
  }
  *out = ws.tile_ctr + (size_t)(*ctr_block)++ * (kTileCtrBytes / sizeof(unsigned));
  return SN_OK;
}

// Hierarchical model (SURVEY.md appendix A `multi`), coarse part, once per low-resolution piece [p0, p0+m): the image
// pyramid of the left eye, then the towers of levels levels-1 .. 1, each starting from the x2 upsample of the map below
// it (the soft-argmin map for the coarsest), values x2, normalised by D / 2^level.  Level k runs in chunks of
// ws.rbk[k] pairs.  Leaves the level-1 maps of the piece in ws.lvl_disp[1].  *ctr_block: next free tile-queue block.
int refine_coarse(sn_handle* h, Workspace& ws, hipStream_t st, int p0, int m, const int8_t* in6, int* ctr_block, int mode) {
  const size_t HW = (size_t)h->H * h->W;
  const int8_t* in_piece = in6 + (size_t)p0 * 6 * HW;
  for (int lv = 1; lv < h->levels; ++lv) {       // level 1 from the int8 input, the others from the level above
    const Tower& T = h->tw[lv];
    if (lv == 1)
      HIP_TRY(h, launch_img_pool2(st, true, in_piece, h->H, h->W, T.Hk, T.Wk, ws.pyr[lv], m));
    else
      HIP_TRY(h, launch_img_pool2(st, false, ws.pyr[lv - 1], 0, 0, T.Hk, T.Wk, ws.pyr[lv], m));
  }
  const float* src = ws.disp_low + (size_t)p0 * h->hl * h->wl;
  int sh = h->hl, sw = h->wl;
  for (int lv = h->levels - 1; lv >= 1; --lv) {
    const Tower& T = h->tw[lv];
    const size_t HWk = (size_t)T.Hk * T.Wk;
    const float dnorm = (float)h->D / (float)(1 << lv);
    const int rbk = chunk_pairs(h, ws, mode, lv);
    for (int q = 0; q < m; q += rbk) {
      const int c = (m - q) < rbk ? (m - q) : rbk;
      RefineCall a{};
      int rc = take_ctr_block(h, ws, ctr_block, &a.chunk_ctr);
      if (rc) return rc;
      a.T = &T;
      a.ref = ws.ref_lv[lv], a.ref16 = ws.ref16_lv[lv];
      a.src = src + (size_t)q * sh * sw, a.sh = sh, a.sw = sw, a.ups = UpScale{0.5f, 2.0f};
      a.img_src = ws.pyr[lv] + (size_t)q * 3 * HWk, a.pyr = true;
      a.H = T.Hk, a.W = T.Wk, a.dnorm = dnorm;
      a.od = ws.lvl_disp[lv] + (size_t)q * HWk;       // (no wire map, no profiling events below level 0)
      a.c = c, a.cap = ws.rbk[lv], a.mode = mode;
      a.stat = ws.stats + (size_t)lv * kStatWordStride;
      if ((rc = refine_level(h, ws, st, a))) return rc;
    }
    src = ws.lvl_disp[lv];
    sh = T.Hk;
    sw = T.Wk;
  }
  return SN_OK;
}

// Full-resolution refinement of ONE tower chunk: pairs [q0, q0+c), c <= ws.rb, of the piece that starts at p0, on
// stream `st` with the activation pair of tower stream `sidx`; *ctr_block: next free tile-queue block.
//   single-scale model: x16 upsample of the soft-argmin map;
//   hierarchical model: x2 upsample of the piece's level-1 maps (refine_coarse ran before on the same stream).
int refine_chunk(sn_handle* h, Workspace& ws, hipStream_t st, int sidx, int* ctr_block, int p0, int q0, int c,
                 const int8_t* in6, float* out_disp, int32_t* out_raw, bool pe, int mode) {
  const int hl = h->hl, wl = h->wl;
  const size_t HW = (size_t)h->H * h->W;
  RefineCall a{};
  if (const int rc = take_ctr_block(h, ws, ctr_block, &a.chunk_ctr)) return rc;
  a.T = &h->tw[0];
  a.ref = &ws.ref[2 * sidx], a.ref16 = &ws.ref16[2 * sidx];
  if (h->levels > 1) {
    a.sh = h->tw[1].Hk, a.sw = h->tw[1].Wk;
    a.src = ws.lvl_disp[1] + (size_t)(q0 - p0) * a.sh * a.sw;
    a.ups = UpScale{0.5f, 2.0f};
  } else {
    a.sh = hl, a.sw = wl;
    a.src = ws.disp_low + (size_t)q0 * hl * wl;
    a.ups = UpScale{1.0f / 16.0f, 16.0f};
  }
  a.img_src = in6 + (size_t)q0 * 6 * HW, a.pyr = false;
  a.H = h->H, a.W = h->W, a.dnorm = (float)h->D;
  a.od = out_disp ? out_disp + (size_t)q0 * HW : nullptr;
  a.orw = out_raw ? out_raw + (size_t)q0 * HW : nullptr;
  a.c = c, a.cap = ws.rb, a.pe = pe, a.mode = mode, a.stat = ws.stats;
  return refine_level(h, ws, st, a);
}

// in6: device int8 [n][6][H][W]; out_disp / out_raw: device, nullable.
// The batch is cut into pieces of ws.pb pairs and every piece into tower chunks of ws.rb pairs.  More than one chunk:
// three streams forked from / joined back into the caller's stream with events (plain stream semantics for the caller):
//   s_low      the low-resolution branch of piece k+1 (matrix-pipe bound, little HBM traffic) runs under
//   s_tow[0/1] the refinement towers of piece k (HBM bound); consecutive chunks ALTERNATE between the two tower
//              streams.  A tower launch costs bytes / 7.5 TB/s plus ~14 us that do not depend on its size (kernel
//              boundary, weight / first-tile prologue, and a tail in which the last tiles of the persistent grid
//              finish one by one); with two independent chunks in flight the workgroups of chunk B's launch take over
//              the CUs that chunk A's launch drains, and A's next launch (which depends only on A) is ready by the
//              time B drains.  Two one-pair chunks in flight = four 61 MB tensors = the footprint of one two-pair
//              chunk, still inside the 256 MB Infinity Cache.
// mode: the arithmetic of this call (SN_PREC_F16 / F16X3 / FP32; 0 = the handle's current one).  Ends with the copy of the
// refinement statistic to the workspace's pinned twin, in stream order.
int forward(sn_handle* h, Workspace& ws, hipStream_t st, int n, const int8_t* in6, float* out_disp,
            int32_t* out_raw, bool want_cost, int mode = 0, bool want_conf = false) {
  if (mode == 0) mode = h->precision == SN_PREC_AUTO ? h->actl.st.mode : h->precision;
  const int rb = chunk_pairs(h, ws, mode);
  const bool prof = h->profiling && (&ws == &h->ws);
  const bool piped = !prof && (&ws == &h->ws) && h->overlap && n > rb;
  int rc;
  int ctr_block = 0;          // tile-queue blocks are handed out in launch order (alloc_ws sized the pool)
  // the tile queues belong to the per-layer fp16 kernel (k_ref_conv_f16_v2): with every block of this call streamed (the
  // default) or on split operands nobody reads them, and the fill is a 4 us launch of its own in front of a single pair
  bool need_queues = ws.tile_ctr != nullptr && mode == SN_PREC_F16;
  if (need_queues && h->fuse_mode == 4) {
    need_queues = false;
    for (int i = 0; i < kNRefRes; ++i) need_queues = need_queues || !stream_block_supports(kRefDil[i]);
  }
  if (need_queues) HIP_TRY(h, hipMemsetAsync(ws.tile_ctr, 0, kTileCtrBytes * ws.n_chunks, st));
  HIP_TRY(h, hipMemsetAsync(ws.stats, 0, kMaxLevels * kStatWordStride * sizeof(unsigned long long), st));
  auto finish = [&]() -> int {
    HIP_TRY(h, hipMemcpyAsync(ws.stats_host, ws.stats, (size_t)h->levels * kStatWordStride * sizeof(unsigned long long),
                              hipMemcpyDeviceToHost, st));        // the levels this model has (2 KB each)
    return SN_OK;
  };
  if (!piped) {
    if (prof) HIP_TRY(h, hipEventRecord(h->ev[0], st));
    for (int p0 = 0, m = 0; p0 < n; p0 += m) {
      m = (n - p0) < ws.pb ? (n - p0) : ws.pb;
      if ((rc = lowres(h, ws, st, p0, m, in6, want_cost, want_conf, prof && p0 == 0))) return rc;
      if (prof && p0 == 0) HIP_TRY(h, hipEventRecord(h->ev[2], st));
      if (h->levels > 1 && (rc = refine_coarse(h, ws, st, p0, m, in6, &ctr_block, mode))) return rc;
      for (int q0 = p0; q0 < p0 + m; q0 += rb) {
        const int c = (p0 + m - q0) < rb ? (p0 + m - q0) : rb;
        if ((rc = refine_chunk(h, ws, st, 0, &ctr_block, p0, q0, c, in6, out_disp, out_raw, prof && q0 == 0, mode))) return rc;
      }
    }
    if (prof) HIP_TRY(h, hipEventRecord(h->ev[3], st));
    return finish();
  }
  const int ns = ws.ns;
  HIP_TRY(h, hipEventRecord(h->ev_fork, st));
  HIP_TRY(h, hipStreamWaitEvent(h->s_low, h->ev_fork, 0));
  for (int s = 0; s < ns; ++s) HIP_TRY(h, hipStreamWaitEvent(h->s_tow[s], h->ev_fork, 0));
  int k = 0, chunk = 0;
  for (int p0 = 0, m = 0; p0 < n; p0 += m, ++k) {
    m = p0 == 0 ? first_piece(h, ws, n) : ((n - p0) < ws.pb ? (n - p0) : ws.pb);
    // the piece-local low-res buffers are reused by the next piece: only disp_low (and conf_low, read after the join) cross streams
    if ((rc = lowres(h, ws, h->s_low, p0, m, in6, want_cost, want_conf, false))) return rc;
    hipEvent_t e = h->ev_piece[k % kMaxPieceEvents];
    HIP_TRY(h, hipEventRecord(e, h->s_low));
    bool waited[kMaxTowerStreams] = {};
    if (h->levels > 1) {                   // coarse levels of the whole piece first (one tower stream: alloc_ws)
      HIP_TRY(h, hipStreamWaitEvent(h->s_tow[0], e, 0));
      waited[0] = true;
      if ((rc = refine_coarse(h, ws, h->s_tow[0], p0, m, in6, &ctr_block, mode))) return rc;
    }
    for (int q0 = p0; q0 < p0 + m; q0 += rb, ++chunk) {
      const int c = (p0 + m - q0) < rb ? (p0 + m - q0) : rb;
      const int s = chunk % ns;
      if (!waited[s]) {
        HIP_TRY(h, hipStreamWaitEvent(h->s_tow[s], e, 0));
        waited[s] = true;
      }
      if ((rc = refine_chunk(h, ws, h->s_tow[s], s, &ctr_block, p0, q0, c, in6, out_disp, out_raw, false, mode))) return rc;
    }
  }
  HIP_TRY(h, hipEventRecord(h->ev_join, h->s_low));
  HIP_TRY(h, hipStreamWaitEvent(st, h->ev_join, 0));
  for (int s = 0; s < ns; ++s) {
    HIP_TRY(h, hipEventRecord(h->ev_tow_join[s], h->s_tow[s]));
    HIP_TRY(h, hipStreamWaitEvent(st, h->ev_tow_join[s], 0));
  }
  return finish();
}

int collect_profile(sn_handle* h) {
  if (!h->profiling) return SN_OK;
  HIP_TRY(h, hipEventSynchronize(h->ev[3]));
  float ms = 0.f;
  HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  h->stage_ms[SN_STAGE_FEATURES] = ms;
  HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[1], h->ev[2]));
  h->stage_ms[SN_STAGE_AGGREGATE] = ms;
  HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[2], h->ev[3]));
  h->stage_ms[SN_STAGE_REFINE] = ms;
  HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[4], h->ev[5]));
  h->stage_ms[SN_STAGE_REFINE_CONV] = ms;    // first refinement chunk only
  HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[3]));
  h->stage_ms[SN_STAGE_TOTAL] = ms;
  // the dominant kernel's launches of the first chunk: the streamed blocks one by one, else the tower span
  if (h->dom_pairs > 0) {
    float sum = 0.f;
    for (int i = 0; i < h->dom_pairs; ++i) {
      HIP_TRY(h, hipEventElapsedTime(&ms, h->ev_dom[2 * i], h->ev_dom[2 * i + 1]));
      sum += ms;
    }
    h->stage_ms[SN_STAGE_DOMINANT] = sum;
  } else {
    h->stage_ms[SN_STAGE_DOMINANT] = h->stage_ms[SN_STAGE_REFINE_CONV];
  }
  return SN_OK;
}

// ---- refinement statistic and SN_PREC_AUTO (include/stereonet_hip.h) ---------------------------------------------------
__global__ __launch_bounds__(256) void k_abs_diff_sum(const float* __restrict__ a, const float* __restrict__ b, size_t n,
                                                      unsigned long long* __restrict__ out) {
  float sum = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) sum += fabsf(a[i] - b[i]);
  refine_stat_commit_block(out, sum);
}

// mean |D_k r_k| per level from a workspace's pinned statistic of an n-pair call (valid once the stream that ran forward()
// has been synchronised): level 0 writes the H x W output maps, a coarse level its whole padded map
// `at`: 0 = the sums, kStatNonfinite / kStatNonfiniteLow = the range check's counts in the same lines
inline unsigned long long stat_word(const Workspace& ws, int word, int at = 0) {      // the word's partial sums (refine_stat_commit)
  unsigned long long sum = 0;
  for (int s = 0; s < kStatSlots; ++s) sum += ws.stats_host[(size_t)word * kStatWordStride + (size_t)s * kStatLine + at];
  return sum;
}
// A non-zero count of the range check makes the residual +inf: whatever the sums say, the fp16 storage is not to be trusted
// with this call (sn_auto_observe then leaves SN_PREC_F16).
void read_stats(const sn_handle* h, const Workspace& ws, int n, double* level_px, double* residual_px, RangeCount* range) {
  double res = 0.0;
  *range = RangeCount{};
  for (int lv = 0; lv < kMaxLevels; ++lv) {
    level_px[lv] = 0.0;
    if (lv >= h->levels || n <= 0) continue;
    const double px = lv == 0 ? (double)h->H * h->W : (double)h->tw[lv].Hk * h->tw[lv].Wk;
    level_px[lv] = (double)stat_word(ws, lv) / (double)kStatScale / (px * n);
    res += level_px[lv] * (double)(1 << lv);
    range->level[lv] = stat_word(ws, lv, kStatNonfinite);
  }
  if (n > 0) range->low = stat_word(ws, 0, kStatNonfiniteLow);
  *residual_px = range->any() ? (double)INFINITY : res;
}
// what a blocking call whose maps come from a flagged arithmetic returns instead of SN_OK
int range_result(sn_handle* h, const RangeCount& r) {
  if (!r.any()) return SN_OK;
  char msg[256];
  snprintf(msg, sizeof msg, "activations left the range of fp16 (65504): non-finite pixels per level %llu/%llu/%llu/%llu, low-resolution "
           "%llu; the maps are not valid — use SN_PREC_FP32 for this model", r.level[0], r.level[1], r.level[2], r.level[3], r.low);
  set_err(h, msg);
  return SN_ERR_RANGE;
}

// every call is counted when it is issued (the statistic of an enqueue-only call may be superseded by the next call's before
// anybody looks at it; the count may not)
void count_call(sn_handle* h, int n) {
  std::lock_guard<std::mutex> lk(h->mu);
  ++h->actl.calls;
  h->actl.pairs += (uint64_t)n;
}

// Folds the statistic of one finished call (run in `mode`) into the handle; returns the arithmetic the handle is in
// afterwards.  observe = false: a repeated call (its first run has been observed already).
int fold_stats(sn_handle* h, const double* level_px, double residual_px, const RangeCount& range, int n, int mode,
               bool observe = true) {
  std::lock_guard<std::mutex> lk(h->mu);
  AutoCtl& a = h->actl;
  for (int lv = 0; lv < kMaxLevels; ++lv) a.last_level[lv] = level_px[lv];
  a.last_res = residual_px;
  a.last_range = range;
  a.last_mode = mode;
  if (!observe) {
    ++a.reruns;
    return a.st.mode;
  }
  if (h->precision != SN_PREC_AUTO) {
    const double r = residual_px <= kAutoResidualCap ? residual_px : kAutoResidualCap;     // as sn_auto_observe
    a.st.running_px = a.st.running_px < 0.0 ? r : 0.75 * a.st.running_px + 0.25 * r;
    return h->precision;
  }
  const int before = a.st.mode;
  const int after = sn_auto_observe(&a.st, residual_px);
  if (before == SN_PREC_F16X3 && after == SN_PREC_F16) a.calibrated = false;      // re-entering F16: check it again
  return after;
}

// SN_PREC_AUTO's self-check: ONE pair in both arithmetics (the low-resolution branch is the same code, so the maps differ by
// the towers' arithmetic alone), mean |F16 - F16X3| against the pair's residual -> the handle's measured EPE per pixel of
// residual.  Runs on `st` with the workspace of the call that triggers it and returns after synchronising.
int auto_selfcheck(sn_handle* h, Workspace& ws, hipStream_t st, const int8_t* in6_pair) {
  std::lock_guard<std::mutex> cal(h->mu_cal);
  {
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->actl.calibrated) return SN_OK;
  }
  const bool prof = h->profiling;
  h->profiling = false;                  // the stage events belong to the caller's own forward()
  double lvl[kMaxLevels], res = 0.0;
  RangeCount range_x3, range;
  int rc = forward(h, ws, st, 1, in6_pair, h->chk[1], nullptr, false, SN_PREC_F16X3);
  if (!rc && hipStreamSynchronize(st) == hipSuccess) read_stats(h, ws, 1, lvl, &res, &range_x3);   // (the next forward clears the words)
  if (!rc) rc = forward(h, ws, st, 1, in6_pair, h->chk[0], nullptr, false, SN_PREC_F16);    // last: the intermediates sn_dbg_read sees
  h->profiling = prof;
  if (rc) return rc;
  const size_t HW = (size_t)h->H * h->W;
  HIP_TRY(h, hipMemsetAsync(ws.stats + 4 * kStatWordStride, 0, kStatWordStride * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_abs_diff_sum, dim3(512), dim3(256), 0, st, h->chk[0], h->chk[1], HW, ws.stats + 4 * kStatWordStride);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipMemcpyAsync(ws.stats_host, ws.stats, kStatU64 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(h, hipStreamSynchronize(st));
  read_stats(h, ws, 1, lvl, &res, &range);
  // a pair that left the range of fp16 in either arithmetic measures nothing (its NaN pixels were clamped to 0 in both maps:
  // their difference would read as an EPE of 0): the handle stays uncalibrated
  if (range.any() || range_x3.any() || stat_word(ws, 4, kStatNonfinite) != 0) return SN_OK;
  const double epe = (double)stat_word(ws, 4) / (double)kStatScale / (double)HW;
  std::lock_guard<std::mutex> lk(h->mu);
  AutoCtl& a = h->actl;
  a.selfcheck_epe = epe;
  a.selfcheck_res = res;
  // (a model whose refinement adds nothing has nothing to lose in fp16: keep the envelope alone)
  a.st.epe_per_px = res > 1e-6 ? epe / res : 0.0;
  a.calibrated = true;
  return SN_OK;
}

// A statistic of an earlier call that only enqueued its work (device buffers + caller stream): folded in once its copy has
// landed (wait = false: only if it already has; wait = true: after waiting for it).  The pending fields are read and
// cleared under h->mu; the event is waited for outside it.
int fold_pending(sn_handle* h, bool wait) {
  AutoCtl& a = h->actl;
  {
    std::lock_guard<std::mutex> lk(h->mu);
    if (!a.pending) return SN_OK;
  }
  if (wait) {
    HIP_TRY(h, hipEventSynchronize(h->ev_stats));
  } else if (hipEventQuery(h->ev_stats) != hipSuccess) {
    (void)hipGetLastError();               // hipErrorNotReady: try again at the next call
    return SN_OK;
  }
  int n, mode;
  {
    std::lock_guard<std::mutex> lk(h->mu);
    if (!a.pending) return SN_OK;
    a.pending = false;
    n = a.pending_n;
    mode = a.pending_mode;
  }
  double lvl[kMaxLevels], res = 0.0;
  RangeCount range;
  read_stats(h, h->ws, n, lvl, &res, &range);
  fold_stats(h, lvl, res, range, n, mode);
  return SN_OK;
}

// What a finished call owes the handle: n pairs from in6, run in `mode` on ws / st and synchronised.  Reads the statistic;
// check (an SN_PREC_AUTO call in SN_PREC_F16): the self-check first, if the handle is uncalibrated and the call was not flagged
// (a flagged call owes none: there is nothing to calibrate on, and the next F16 call of the handle, if any, has it); count: the
// caller has not counted the call yet (sn_wait: a request counts once its self-check has passed); folds; and a call the fold
// sends out of the fp16 tower's envelope is REPEATED: rerun() runs it again in SN_PREC_F16X3 with whatever the caller enqueues
// behind it and returns once that has completed; its statistic is folded in without being observed a second time.
// *range: the counts of the arithmetic whose maps the caller holds afterwards.
template <class Rerun>
int settle(sn_handle* h, Workspace& ws, hipStream_t st, int n, const int8_t* in6, int mode, bool check, bool count,
           Rerun rerun, RangeCount* range) {
  double lvl[kMaxLevels], res = 0.0;
  int rc;
  read_stats(h, ws, n, lvl, &res, range);
  if (check && !range->any() && (rc = auto_selfcheck(h, ws, st, in6))) return rc;
  if (count) count_call(h, n);
  const int next = fold_stats(h, lvl, res, *range, n, mode);
  if (h->precision == SN_PREC_AUTO && mode == SN_PREC_F16 && next == SN_PREC_F16X3) {
    if ((rc = rerun())) return rc;
    read_stats(h, ws, n, lvl, &res, range);
    fold_stats(h, lvl, res, *range, n, SN_PREC_F16X3, false);
  }
  return SN_OK;
}

// forward() on the handle's own workspace for the synchronous entry points.  post() enqueues what follows the network
// (device-to-host copies; sn_infer_conf: the confidence kernel, which reads ws.conf_low — want_conf — and the maps after the
// towers have joined, and runs again after a repeat so that its outputs belong to the arithmetic that returned).
// blocking: the entry point returns after completion, so the call is settled before it does; maps that come from an
// arithmetic that left the range of fp16 return SN_ERR_RANGE (range_result).  Not blocking (work only enqueued on the caller's
// stream): the statistic is folded in by a later call; an AUTO handle that has not had its self-check yet blocks once.
// A blocking call WAITS for the statistic of an enqueue-only call before it (its own forward overwrites the pinned words:
// left pending, they would later be read as that earlier call's and divided by its n).
template <class Post>
int run_forward(sn_handle* h, hipStream_t st, int n, const int8_t* din, float* ddisp, int32_t* draw, bool want_cost,
                bool blocking, Post post, bool want_conf = false) {
  const bool is_auto = h->precision == SN_PREC_AUTO;
  AutoCtl& a = h->actl;
  int rc = fold_pending(h, blocking);
  if (rc) return rc;
  int mode, calibrated;
  {
    std::lock_guard<std::mutex> lk(h->mu);
    mode = is_auto ? a.st.mode : h->precision;
    calibrated = a.calibrated;
  }
  const bool check = is_auto && mode == SN_PREC_F16 && !calibrated;
  if ((rc = forward(h, h->ws, st, n, din, ddisp, draw, want_cost, mode, want_conf))) return rc;
  if ((rc = post())) return rc;
  count_call(h, n);
  if (!blocking && !check) {
    HIP_TRY(h, hipEventRecord(h->ev_stats, st));
    std::lock_guard<std::mutex> lk(h->mu);
    a.pending = true;
    a.pending_n = n;
    a.pending_mode = mode;
    return SN_OK;
  }
  HIP_TRY(h, hipStreamSynchronize(st));
  RangeCount range;
  auto rerun = [&]() -> int {
    int r = forward(h, h->ws, st, n, din, ddisp, draw, want_cost, SN_PREC_F16X3, want_conf);
    if (!r) r = post();
    if (r) return r;
    HIP_TRY(h, hipStreamSynchronize(st));
    return SN_OK;
  };
  if ((rc = settle(h, h->ws, st, n, din, mode, check, false, rerun, &range))) return rc;
  if ((rc = collect_profile(h))) return rc;
  return blocking ? range_result(h, range) : SN_OK;      // the counts of the arithmetic whose maps the caller holds
}

}  // namespace
