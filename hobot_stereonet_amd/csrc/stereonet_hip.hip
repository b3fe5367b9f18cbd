// stereonet_hip.hip — the one translation unit of the engine of libstereonet_hip.so: the headers below, one concern each and
// included in order, then the public C ABI (include/stereonet_hip.h): create, destroy, infer, submit / wait, preprocess,
// measurement, depth, point cloud, left-right check.  DESIGN.md §6 has the source map.
//
// Replaces, for the StereoNet hot path, what the reference obtains from the closed dnn_node /
// libdnn runtime: model load (DnnNode::Init, stereonet_infer/src/stereonet_node.cpp:44), tensor
// introspection (:57-103) and DnnNode::Run (:812 async, :968 sync).  No CPU fallback exists: if
// there is no gfx950 device every entry point fails with SN_ERR_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>

#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/stereonet_hip.h"
#include "sn_internal.h"
#include "sn_switches.hpp"      // the SN_* environment switches
#include "sn_kernels.hpp"       // device code (with sn_pointcloud.hpp, sn_lrcheck.hpp, sn_dispfilter.hpp, sn_confidence.hpp)
#include "sn_pointcloud.hpp"
#include "sn_lrcheck.hpp"
#include "sn_dispfilter.hpp"
#include "sn_confidence.hpp"
#include "sn_engine.hpp"        // handle, workspace and layer types, error and allocation helpers
#include "sn_weights.hpp"       // .snw reader, weight packing and upload
#include "sn_launch.hpp"        // kernel launchers and tensor geometry
#include "sn_forward.hpp"       // workspace allocation, forward pass, refinement statistic, SN_PREC_AUTO
#include "sn_dbg_hooks.hpp"     // sn_dbg_* parity hooks

// =====================================================================================================
// C ABI
// =====================================================================================================
extern "C" {

const char* sn_strerror(int code) {
  switch (code) {
    case SN_OK: return "ok";
    case SN_ERR_ARG: return "invalid argument";
    case SN_ERR_FILE: return "model file missing or unreadable";
    case SN_ERR_FORMAT: return "model file is not an SN-K4 SNW1 weight file";
    case SN_ERR_DEVICE: return "HIP device error (a gfx950 GPU is required; there is no CPU path)";
    case SN_ERR_NOMEM: return "out of memory";
    case SN_ERR_BUSY: return "no free task slot";
    case SN_ERR_TICKET: return "unknown ticket";
    default: return "unknown error";
  }
}

// detail of the last failed sn_create on this thread (there is no handle to carry it)
static thread_local std::string g_create_err;
static int create_fail(int code, const char* what) {
  const hipError_t e = hipGetLastError();
  g_create_err = std::string(what) + (e != hipSuccess ? std::string(": ") + hipGetErrorString(e) : std::string());
  return code;
}

const char* sn_last_error(const sn_handle* h) {
  if (!h) return g_create_err.c_str();
  thread_local std::string copy;      // the caller's own copy: another thread's failure cannot change it under the caller
  std::lock_guard<std::mutex> lk(h->err_mu);
  copy = h->err;
  return copy.c_str();
}

int sn_create(const char* model_file, const sn_config* cfg, sn_handle** out) {
  return sn_create_prio(model_file, cfg, -1, out);
}

// stream_prio: 1 = pipeline streams at the device's highest priority, 0 = default priority, -1 = SN_STREAM_PRIORITY decides
// (unset: default).  An explicit SN_STREAM_PRIORITY always wins, so the A/B switch stays usable for every caller.
int sn_create_prio(const char* model_file, const sn_config* cfg, int stream_prio, sn_handle** out) {
  if (!model_file || !out) return SN_ERR_ARG;
  *out = nullptr;
  FILE* f = fopen(model_file, "rb");
  if (!f) return SN_ERR_FILE;
  SnwHeader hd;
  if (fread(&hd, 1, sizeof hd, f) != sizeof hd || memcmp(hd.magic, "SNW1", 4) != 0) {
    fclose(f);
    return SN_ERR_FORMAT;
  }
  const uint32_t dil_ok[6] = {1, 2, 4, 8, 1, 1};
  if (hd.version != 1 || hd.channels != kC || hd.n_down != kNDown || hd.n_fres != kNFeatRes ||
      hd.n_agg != kNAgg || hd.n_rres != kNRefRes || memcmp(hd.dil, dil_ok, sizeof dil_ok) != 0 ||
      (hd.reserved != 0 && hd.reserved != 1 && hd.reserved != (uint64_t)kMultiLevels)) {
    fclose(f);
    return SN_ERR_FORMAT;
  }
  // header word 72: refinement levels (0 / 1 = single-scale tower, 4 = hierarchical; weights.py documents the layout)
  const int levels = hd.reserved > 1 ? (int)hd.reserved : 1;
  if (hd.n_params != param_count(levels)) {
    fclose(f);
    return SN_ERR_FORMAT;
  }
  std::vector<float> blob(hd.n_params);
  const size_t got = fread(blob.data(), sizeof(float), blob.size(), f);
  fclose(f);
  if (got != blob.size()) return SN_ERR_FORMAT;

  const Switches sw = switches_at_create();      // process-scope switches as latched, create-scope ones as they are now
  sn_config c{};
  if (cfg) c = *cfg; else c.device = -1;
  const int W = c.width > 0 ? c.width : (int)hd.width;
  const int H = c.height > 0 ? c.height : (int)hd.height;
  const int D = c.dmax > 0 ? c.dmax : (int)hd.dmax;
  if (W <= 0 || H <= 0 || D < 16 || D % 16 || D > 256) return SN_ERR_ARG;   // NV12 entry points add w%4, h%2
  if (c.precision == SN_PREC_DEFAULT) {
    // SN_PRECISION=f16|f16x3|fp32|auto: what "default" means for this process (A/B runs of unmodified callers)
    c.precision = sw.precision;
  }
  if (c.precision != SN_PREC_FP32 && c.precision != SN_PREC_F16 && c.precision != SN_PREC_F16X3 && c.precision != SN_PREC_AUTO)
    return SN_ERR_ARG;

  int ndev = 0;
  g_create_err.clear();
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return create_fail(SN_ERR_DEVICE, "hipGetDeviceCount");
  int dev = c.device;
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return create_fail(SN_ERR_DEVICE, "hipGetDevice");
  if (dev >= ndev) return SN_ERR_ARG;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return create_fail(SN_ERR_DEVICE, "hipGetDeviceProperties");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    fprintf(stderr, "stereonet_hip: device %d is %s, this library is built for gfx950 only\n", dev,
            prop.gcnArchName);
    return SN_ERR_DEVICE;
  }

  sn_handle* h = new sn_handle();
  h->device = dev;
  h->W = W;
  h->H = H;
  h->D = D;
  h->Wp = (W + 15) / 16 * 16;
  h->Hp = (H + 15) / 16 * 16;
  h->wl = h->Wp / 16;
  h->hl = h->Hp / 16;
  h->Dl = D / 16;
  h->max_batch = c.max_batch > 0 ? c.max_batch : 1;
  h->precision = c.precision;
  h->task_num = c.task_num > 0 ? c.task_num : 4;
  h->refine_chunk = c.refine_chunk;                            // <= 0: chosen below from the tensor size
  h->piece = c.piece > 0 ? c.piece : 16;
  h->levels = levels;
  sn_auto_init(&h->actl.st, levels);
  if (c.precision != SN_PREC_AUTO) h->actl.st.mode = c.precision;
  h->actl.last_mode = h->actl.st.mode;
  for (int k = 0; k < levels; ++k) {
    h->tw[k].Hk = h->Hp >> k;
    h->tw[k].Wk = h->Wp >> k;
    h->tw[k].rg = make_ref_geom(h->tw[k].Hk, h->tw[k].Wk);
  }
  {
    // SN_TOWER_STREAMS: 2 = consecutive tower chunks alternate between two streams
    // default 1; 2 in SN_PREC_FP32: a one-pair launch of the fp32 tower kernel is 3.5 rounds of tiles on the persistent
    // grid, and the next chunk's launch on the other stream takes the CUs the last half round leaves idle (+6 %)
    h->tower_streams = sw.tower_streams != kSwitchUnset ? sw.tower_streams : (h->precision == SN_PREC_FP32 ? 2 : 1);
    if (h->tower_streams < 1) h->tower_streams = 1;
    if (h->tower_streams > kMaxTowerStreams) h->tower_streams = kMaxTowerStreams;
  }
  const bool want_f16 = c.precision == SN_PREC_F16 || c.precision == SN_PREC_AUTO;
  const bool want_x3 = c.precision == SN_PREC_F16X3 || c.precision == SN_PREC_AUTO;
  {
    // the Infinity-Cache sizing of the per-layer forms, for the split tensors of SN_PREC_F16X3 (what an AUTO handle falls back to)
    const double tensor_mb = 4.0 * h->tw[0].rg.Hs * h->tw[0].rg.Ws * 16.0 / 1048576.0 * 2.0;
    int r = (int)(256.0 / (2.0 * tensor_mb * h->tower_streams) + 0.5);
    // with the split blocks streamed too (sn_stream_block_x3.hpp) the chunk no longer has to live in the Infinity Cache:
    // the fp16 rule below (1280x720: one pair 1067, four 1099-1134, six 1137-1139, eight 1142 pairs/s, profiles/r06_x3_stream_ab.txt)
    if (stream_x3_supports(8)) {
      const int by_px = (int)(5.5e6 / ((double)h->Hp * h->Wp) + 0.5);
      if (by_px > r) r = by_px;
    }
    h->refine_chunk_x3 = r < 1 ? 1 : (r > 8 ? 8 : r);
  }
  if (h->refine_chunk <= 0) {
    // Pairs per tower launch: as many as keep the activations in flight — (x, t) per tower stream — inside the
    // 256 MB Infinity Cache.  A launch costs bytes / ~7 TB/s while its tensors stay cache resident plus ~8 us that do
    // not depend on its size, and ~5 TB/s per byte once they spill (scripts/mall_probe.hip): 1280x720
    // -> 2 pairs (4 x 61 MB), 1248x384 -> 4 pairs (8 x 32 MB); measured equal to one-pair chunks alternating on two
    // streams (SN_TOWER_STREAMS=2), with fewer and fuller launches.
    const double tensor_mb = 4.0 * h->tw[0].rg.Hs * h->tw[0].rg.Ws * 16.0 / 1048576.0 * (c.precision == SN_PREC_F16X3 ? 2.0 : c.precision == SN_PREC_FP32 ? 2.0 : 1.0);
    int rc_auto = (int)(256.0 / (2.0 * tensor_mb * h->tower_streams) + 0.5);
    // With every residual block streamed (fp16 mode, SN_FUSE=4) a launch reads x and writes y ONCE while it does two
    // convolutions: ~2.8 TB/s at the rate the matrix pipes allow, which HBM sustains — the chunk no longer has to live in
    // the Infinity Cache, and fuller launches amortise the restart rows and the launch itself: ~5.5 Mpx per launch
    // (1280x720: 6 pairs; round 3: 4 pairs 2583 -> 2653 pairs/s; round 5, three interleaved runs: 4 pairs 3064-3068,
    // 6 pairs 3074-3081, 8 pairs 3071-3078, profiles/r05_schedule_sweep.txt).
    if ((want_f16 && sw.fuse == 4 && stream_block_supports(8)) || (c.precision == SN_PREC_F16X3 && stream_x3_supports(8))) {
      const int by_px = (int)(5.5e6 / ((double)h->Hp * h->Wp) + 0.5);
      if (by_px > rc_auto) rc_auto = by_px;
    }
    h->refine_chunk = rc_auto < 1 ? 1 : (rc_auto > 8 ? 8 : rc_auto);
  }
  h->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (h->refine_chunk > h->max_batch) h->refine_chunk = h->max_batch;
  if (h->refine_chunk_x3 > h->refine_chunk) h->refine_chunk_x3 = h->refine_chunk;

  // the kernels use 32-bit element / byte offsets inside one tensor: keep every tensor below 2^32
  {
    // with the piece / chunk sizes alloc_ws will really use (a piece is never smaller than a chunk), and for the
    // activation tensor of EVERY refinement level (a coarse level holds up to rb * 4^k pairs of a relatively more
    // padded plane)
    const int pb = piece_pairs(h, h->max_batch, h->refine_chunk);
    const double low_elems = 2.0 * pb * kC * (h->Hp / 2.0) * (h->Wp / 2.0);
    const double vol_elems = (double)pb * h->Dl * kC * h->hl * h->wl;
    double ref_bytes = 0;
    for (int lv = 0; lv < h->levels; ++lv) {
      const RefGeom& rg = h->tw[lv].rg;
      // (SN_PREC_F16X3's lo tensor sits behind the hi tensor; its offset is folded into 64-bit base pointers)
      const double b = ((double)level_chunk_pairs(h->refine_chunk, pb, lv) * 4.0 * rg.Hs * rg.Ws + (double)ref_slack(rg) + (double)ref_front(rg)) * 16.0;
      if (b > ref_bytes) ref_bytes = b;
    }
    if (low_elems >= 4.0e9 || ref_bytes >= 4.0e9 || vol_elems >= 4.0e9) {
      delete h;
      return SN_ERR_ARG;
    }
  }
  int rc = check_device(h);
  auto fail = [&](int code) {
    create_fail(code, h->err.empty() ? "engine set-up" : h->err.c_str());
    sn_destroy(h);
    return code;
  };
  if (rc) return fail(rc);
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return fail(SN_ERR_DEVICE);
  for (auto& e : h->ev)
    if (hipEventCreate(&e) != hipSuccess) return fail(SN_ERR_DEVICE);
  for (auto& e : h->ev_dom)
    if (hipEventCreate(&e) != hipSuccess) return fail(SN_ERR_DEVICE);
  if (hipEventCreateWithFlags(&h->ev_stats, hipEventDisableTiming) != hipSuccess) return fail(SN_ERR_DEVICE);
  if (c.precision == SN_PREC_AUTO)
    for (auto& p : h->chk)
      if (dalloc(&p, (size_t)H * W) != hipSuccess) return fail(SN_ERR_NOMEM);
  // (Disjoint CU sets for the pipeline streams through hipExtStreamCreateWithCUMask were measured and dropped:
  // 1940 pairs/s shared vs 1700 / 1680 / 1510 with 64 / 96 / 128 CUs split off for the low-resolution branch.)
  // High-priority pipeline streams (stream_prio = 1: sn_mgpu_create for its own exchange streams when more than one
  // device takes part; SN_STREAM_PRIORITY=1 / 0 forces it on / off for any caller).  HIP multiplexes streams onto
  // GPU_MAX_HW_QUEUES (4) hardware queues PER PRIORITY LEVEL, and two streams that share a hardware queue run in order: a
  // caller's other streams (a communication library's receive kernels on the gather root, copy streams) can land on the
  // tower's queue and serialise with it.  High-priority streams draw from their own queues.  Not the default for a
  // single engine: the host-to-host paths measured 30 % slower with it.
  int prio = 0;
  {
    int least = 0, greatest = 0;
    const bool want = sw.stream_priority != kSwitchUnset ? sw.stream_priority == 1 : stream_prio == 1;
    if (want && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess) prio = greatest;
  }
  h->stream_prio = prio != 0;
  auto mk_stream = [&](hipStream_t* st) {
    return prio != 0 ? hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio) : hipStreamCreateWithFlags(st, hipStreamNonBlocking);
  };
  if (mk_stream(&h->s_low) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess)
    return fail(SN_ERR_DEVICE);
  for (int i = 0; i < kMaxTowerStreams; ++i)
    if (mk_stream(&h->s_tow[i]) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_tow_join[i], hipEventDisableTiming) != hipSuccess)
      return fail(SN_ERR_DEVICE);
  for (auto& e : h->ev_piece)
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return fail(SN_ERR_DEVICE);
  h->overlap = !sw.no_overlap;
  h->use_graphs = !sw.no_graph;
  h->fuse_mode = sw.fuse;
  h->tail_fuse = sw.tail_fuse;
  if (hipMalloc(reinterpret_cast<void**>(&h->dump), 4096) != hipSuccess) return fail(SN_ERR_NOMEM);

  BlobWalker bw{blob.data()};
  const bool low_x3 = h->precision != SN_PREC_FP32;     // fp16 modes: low-resolution layers on split fp16 operands
  const unsigned abl_w = sw.ablate_w;
#if SN_DIAGNOSTICS
  h->ablate_x = sw.ablate_x;
#endif
  int feat_idx = 0;
  h->fold_down01 = low_x3 && sw.down01;
  HostLayer hl_down0{};
  for (int i = 0; i < kNDown; ++i) {
    const HostLayer hl_ = bw.next(kC, i == 0 ? 3 : kC, 25);
    if ((rc = upload_conv2d(h, hl_, 4, &h->down[i]))) return fail(rc);
    if (low_x3 && i == 0 && (rc = upload_down0_f16(h, hl_, &h->down0))) return fail(rc);
    if (i == 0) hl_down0 = hl_;
    if (h->fold_down01 && i == 1 && (rc = upload_down01(h, hl_down0, hl_, &h->down01))) return fail(rc);
    if (low_x3 && i > 0 &&
        (rc = upload_x3(h, kC, [&](int co, int c, int tap) { return hl_.w[((size_t)co * kC + c) * 25 + tap]; },
                        &h->down[i], 25, (abl_w >> (kAblDown + i - 1)) & 1u)))
      return fail(rc);
  }
  // fp16 modes: the low-resolution 3x3 / 3x3x3 layers also get split fp16 A-fragments (22-bit operands on the
  // fp16 MFMA, k_conv3x3_c32_x3); SN_PREC_FP32 keeps every contraction on the exact-fp32 MFMA
  auto up2d = [&](ConvLayer* L) -> int {
    const HostLayer hl_ = bw.next(kC, kC, 9);
    int r = upload_conv2d(h, hl_, 8, L);
    if (r || !low_x3) return r;
    const bool z = (abl_w >> (kAblFeat + feat_idx)) & 1u;
    ++feat_idx;
    return upload_x3(h, kC, [&](int co, int c, int tap) { return hl_.w[((size_t)co * kC + c) * 9 + tap]; }, L, 9, z);
  };
  for (int i = 0; i < kNFeatRes; ++i)
    for (int j = 0; j < 2; ++j)
      if ((rc = up2d(&h->fres[i][j]))) return fail(rc);
  if ((rc = up2d(&h->fout))) return fail(rc);
  for (int i = 0; i < kNAgg; ++i) {
    const HostLayer hl_ = bw.next(kC, kC, 27);
    if ((rc = upload_conv3d(h, hl_, &h->agg[i]))) return fail(rc);
    if (low_x3 && (rc = upload_x3(h, 96, [&](int co, int c, int tap) {      // c = kz*32 + ci
          return hl_.w[(((size_t)co * kC + (c & 31)) * 3 + (c >> 5)) * 9 + tap];
        }, &h->agg[i], 9, (abl_w >> (kAblAgg + i)) & 1u)))
      return fail(rc);
  }
  {
    const HostLayer hl_ = bw.next(1, kC, 27);
    if ((rc = upload_head(h, hl_, &h->aout))) return fail(rc);
    if (low_x3 && (rc = upload_agg_head_frag(h, hl_, &h->aout))) return fail(rc);
  }
  for (int lv = 0; lv < h->levels; ++lv) {          // blob order: tower of level 0, then (multi) levels 1, 2, 3
    Tower& T = h->tw[lv];
    {
      const HostLayer hl_ = bw.next(kC, 4, 9);
      if ((rc = upload_conv2d(h, hl_, 4, &T.rin))) return fail(rc);
      if (h->precision != SN_PREC_FP32 && (rc = upload_refin_f16(h, hl_, &T.refin))) return fail(rc);
    }
    for (int i = 0; i < kNRefRes; ++i)
      for (int j = 0; j < 2; ++j) {
        const HostLayer hl_ = bw.next(kC, kC, 9);
        if (h->precision == SN_PREC_FP32 && (rc = upload_conv2d(h, hl_, 8, &T.rres[i][j]))) return fail(rc);
        if (want_x3 && (rc = upload_ref_f16x3(h, hl_, &T.rres16x3[i][j]))) return fail(rc);
        if (want_f16 && (rc = upload_ref_f16(h, hl_, sw.w_round_sum_preserving, &T.rres16[i][j]))) return fail(rc);
      }
    if ((rc = upload_head(h, bw.next(1, kC, 9), &T.rout))) return fail(rc);
  }
  if (bw.off != blob.size()) return fail(SN_ERR_FORMAT);

  if ((rc = alloc_ws(h, &h->ws, h->max_batch, h->refine_chunk, h->tower_streams, h->refine_chunk_x3)))
    return fail(rc == SN_ERR_DEVICE ? SN_ERR_NOMEM : rc);
  *out = h;
  return SN_OK;
}

int sn_destroy(sn_handle* h) {
  if (!h) return SN_ERR_ARG;
  hipSetDevice(h->device);
  hipDeviceSynchronize();
  auto free_conv = [](ConvLayer& l) {
    hipFree(l.wx3);
    hipFree(l.wpk);
    hipFree(l.bias);
  };
  for (auto& l : h->down) free_conv(l);
  hipFree(h->down0.wfrag);
  hipFree(h->down01.wfrag);
  hipFree(h->down01.bias);
  for (auto& b : h->fres)
    for (auto& l : b) free_conv(l);
  free_conv(h->fout);
  for (auto& l : h->agg) free_conv(l);
  for (auto& T : h->tw) {
    hipFree(T.refin.wfrag);
    free_conv(T.rin);
    for (auto& b : T.rres)
      for (auto& l : b) free_conv(l);
    for (auto& b : T.rres16)
      for (auto& l : b) {
        hipFree(l.wfrag);
        hipFree(l.bias);
      }
    for (auto& b : T.rres16x3)
      for (auto& l : b) {
        hipFree(l.wfrag);
        hipFree(l.bias);
      }
    hipFree(T.rout.w);
  }
  hipFree(h->dump);
  hipFree(h->pc.scratch);
  for (void* p : h->pc.dev) hipFree(p);
  for (void* p : h->pc.pin)
    if (p) hipHostFree(p);
  if (h->pc.ev) hipEventDestroy(h->pc.ev);
  if (h->pc.stream) hipStreamDestroy(h->pc.stream);
  for (void* p : h->lrc.dev) hipFree(p);
  hipFree(h->flt.scratch);
  for (void* p : h->flt.dev) hipFree(p);
  if (h->flt.ev) hipEventDestroy(h->flt.ev);
  if (h->flt.stream) hipStreamDestroy(h->flt.stream);
  hipFree(h->aout.w);
  hipFree(h->aout.pfrag);
  for (auto p : h->chk) hipFree(p);
  if (h->ev_stats) hipEventDestroy(h->ev_stats);
  free_ws(&h->ws);
  for (auto& s : h->slots) {
    free_ws(&s.ws);
    if (s.pin_in) hipHostFree(s.pin_in);
    if (s.pin_raw) hipHostFree(s.pin_raw);
    if (s.pin_disp) hipHostFree(s.pin_disp);
    for (auto& gk : s.gexec)
      for (auto& gm : gk)
        for (auto& g : gm)
          if (g) hipGraphExecDestroy(g);
    if (s.ev0) hipEventDestroy(s.ev0);
    if (s.ev1) hipEventDestroy(s.ev1);
    if (s.stream) hipStreamDestroy(s.stream);
  }
  for (auto& e : h->ev)
    if (e) hipEventDestroy(e);
  for (auto& e : h->ev_dom)
    if (e) hipEventDestroy(e);
  for (auto& e : h->ev_piece)
    if (e) hipEventDestroy(e);
  if (h->ev_fork) hipEventDestroy(h->ev_fork);
  if (h->ev_join) hipEventDestroy(h->ev_join);
  if (h->s_low) hipStreamDestroy(h->s_low);
  for (auto& st : h->s_tow)
    if (st) hipStreamDestroy(st);
  for (auto& e : h->ev_tow_join)
    if (e) hipEventDestroy(e);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
  return SN_OK;
}

int sn_get_io_info(const sn_handle* h, sn_io_info* info) {
  if (!h || !info) return SN_ERR_ARG;
  memset(info, 0, sizeof *info);
  info->width = h->W;
  info->height = h->H;
  info->dmax = h->D;
  info->in_channels = 6;
  info->max_batch = h->max_batch;
  info->precision = h->precision;
  info->task_num = h->task_num;
  info->device = h->device;
  info->out_scale = kOutScale;
  info->in_bytes = (size_t)6 * h->H * h->W;
  info->out_bytes = (size_t)4 * h->H * h->W;
  double mac = 0;
  const double wp = h->Wp, hp = h->Hp, wl = h->wl, hl = h->hl, dl = h->Dl;
  for (int k = 1; k <= kNDown; ++k) mac += 2.0 * (wp * hp / (double)(1 << (2 * k))) * kC * (k == 1 ? 3 : kC) * 25;
  mac += 2.0 * (2 * kNFeatRes + 1) * wl * hl * kC * kC * 9;
  mac += kNAgg * dl * hl * wl * kC * kC * 27 + dl * hl * wl * kC * 27;
  for (int k = 0; k < h->levels; ++k)
    mac += (wp * hp / (double)(1 << (2 * k))) * (4.0 * kC * 9 + 2.0 * kNRefRes * kC * kC * 9 + kC * 9);
  info->flops_per_pair = 2.0 * mac;
  info->refine_levels = h->levels;
  info->precision_selected = h->precision == SN_PREC_AUTO ? h->actl.st.mode : h->precision;
  info->refine_chunk = chunk_pairs(h, h->ws, info->precision_selected);
  info->piece = h->ws.pb;
  info->tower_streams = h->ws.ns;
  return SN_OK;
}

int sn_abi_version(void) { return SN_ABI_VERSION; }

// ---- SN_PREC_AUTO's state machine: pure functions, no device (tests/test_auto_precision.py) -------------------------------
// Envelope of the fp16 tower per shape class, in full-resolution pixels of residual_px = sum_k 2^k mean |D_k r_k|: the
// largest value below which EVERY weight draw of the sensitivity tables kept EPE < 1e-3 px against the oracle
// = SN_AUTO_BUDGET_PX over the worst error per pixel of residual of the table (profiles/r06_auto_envelope_*.txt: 8 seeds x
// head gain {1, 2, 4, 8}; single-scale 1280x720: 1.8e-4 .. 8.3e-4 px per px; hierarchical 1242x375: 1.1e-4 .. 2.9e-4 px per
// px of the 2^k-weighted sum — a coarse level's error is upsampled with its map).  The self-check replaces this prior by the
// model's own slope (sn_auto_limit_px).
double sn_auto_envelope_px(int refine_levels) { return refine_levels > 1 ? kAutoEnvelopeMulti : kAutoEnvelopeSingle; }

int sn_auto_init(sn_auto_state* s, int refine_levels) {
  if (!s) return SN_ERR_ARG;
  s->mode = SN_PREC_F16;
  s->calm = 0;
  s->envelope_px = sn_auto_envelope_px(refine_levels);
  s->epe_per_px = 0.0;
  s->running_px = -1.0;
  s->switches = 0;
  return SN_OK;
}

double sn_auto_limit_px(const sn_auto_state* s) {
  if (!s) return 0.0;
  if (!(s->epe_per_px > 0.0)) return s->envelope_px;        // nothing measured on this model yet: the class envelope
  const double cap = SN_AUTO_ENVELOPE_CAP * s->envelope_px, own = SN_AUTO_BUDGET_PX / s->epe_per_px;
  return own < cap ? own : cap;
}

int sn_auto_observe(sn_auto_state* s, double residual_px) {
  if (!s) return SN_ERR_ARG;
  if (!(residual_px >= 0.0)) residual_px = 1e30;       // NaN / negative: nothing the fp16 tower should be trusted with
  s->running_px = s->running_px < 0.0 ? residual_px : 0.75 * s->running_px + 0.25 * residual_px;
  const double lim = sn_auto_limit_px(s);
  if (s->mode == SN_PREC_F16) {
    if (residual_px > lim) {
      s->mode = SN_PREC_F16X3;
      s->calm = 0;
      ++s->switches;
    }
  } else {
    if (residual_px < SN_AUTO_REENTRY * lim) {
      if (++s->calm >= SN_AUTO_CALM_CALLS) {
        s->mode = SN_PREC_F16;
        s->calm = 0;
        ++s->switches;
      }
    } else {
      s->calm = 0;
    }
  }
  return s->mode;
}

int sn_get_refine_stats(sn_handle* h, sn_refine_stats* out) {
  if (!h || !out) return SN_ERR_ARG;
  int rc = check_device(h);
  if (rc) return rc;
  if ((rc = fold_pending(h, true))) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  const AutoCtl& a = h->actl;
  memset(out, 0, sizeof *out);
  out->levels = h->levels;
  out->precision = h->precision;
  out->precision_selected = h->precision == SN_PREC_AUTO ? a.st.mode : h->precision;
  out->precision_last = a.last_mode;
  out->calls = a.calls;
  out->pairs = a.pairs;
  out->switches = a.st.switches;
  out->reruns = a.reruns;
  for (int lv = 0; lv < kMaxLevels; ++lv) out->level_px[lv] = a.last_level[lv];
  out->residual_px = a.last_res;
  out->running_px = a.st.running_px < 0.0 ? 0.0 : a.st.running_px;
  out->envelope_px = a.st.envelope_px;
  out->limit_px = sn_auto_limit_px(&a.st);
  out->selfcheck_epe_px = a.selfcheck_epe;
  out->selfcheck_residual_px = a.selfcheck_res;
  return SN_OK;
}

int sn_infer_batch(sn_handle* h, int n, const int8_t* in, int32_t* out_i32, float* out_disp, int mem,
                   void* stream) {
  if (!h) return SN_ERR_ARG;
  if (!in || (!out_i32 && !out_disp) || n <= 0 || n > h->max_batch || (mem != SN_MEM_HOST && mem != SN_MEM_DEVICE)) {
    set_err(h, "sn_infer_batch: bad arguments");
    return SN_ERR_ARG;
  }
  int rc = check_device(h);
  if (rc) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  const size_t HW = (size_t)h->H * h->W;
  const int8_t* din = in;
  int32_t* draw = out_i32;
  float* ddisp = out_disp;
  if (mem == SN_MEM_HOST) {
    HIP_TRY(h, hipMemcpyAsync(h->ws.in6, in, (size_t)n * 6 * HW, hipMemcpyHostToDevice, st));
    din = h->ws.in6;
    draw = out_i32 ? h->ws.out_raw : nullptr;
    ddisp = out_disp ? h->ws.out_disp : nullptr;
  }
  auto post = [&]() -> int {
    if (mem == SN_MEM_HOST) {
      if (out_i32) HIP_TRY(h, hipMemcpyAsync(out_i32, draw, (size_t)n * HW * 4, hipMemcpyDeviceToHost, st));
      if (out_disp) HIP_TRY(h, hipMemcpyAsync(out_disp, ddisp, (size_t)n * HW * 4, hipMemcpyDeviceToHost, st));
    }
    return SN_OK;
  };
  return run_forward(h, st, n, din, ddisp, draw, n == 1, mem == SN_MEM_HOST || !stream, post);
}

int sn_infer_i8(sn_handle* h, const int8_t* in, int32_t* out_i32, float* out_disp, int mem, void* stream) {
  return sn_infer_batch(h, 1, in, out_i32, out_disp, mem, stream);
}

static int pre_args_ok(sn_handle* h, int w, int hp) { return w == h->W && hp == h->H; }

int sn_preprocess_nv12(sn_handle* h, const uint8_t* left, const uint8_t* right, int w, int h_px,
                       int8_t* out6, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  if (!left || !right || !out6 || w <= 0 || h_px <= 0 || (w & 3) || (h_px & 1) ||
      (size_t)w * h_px > (size_t)h->W * h->H || (mem != SN_MEM_HOST && mem != SN_MEM_DEVICE)) {
    set_err(h, "sn_preprocess_nv12: bad arguments");
    return SN_ERR_ARG;
  }
  int rc = check_device(h);
  if (rc) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  const size_t eye = (size_t)w * h_px * 3 / 2;
  const uint8_t *dl = left, *dr = right;
  int8_t* dout = out6;
  if (mem == SN_MEM_HOST) {
    HIP_TRY(h, hipMemcpyAsync(h->ws.nv12, left, eye, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(h->ws.nv12 + eye, right, eye, hipMemcpyHostToDevice, st));
    dl = h->ws.nv12;
    dr = h->ws.nv12 + eye;
    dout = h->ws.in6;
  } else if (((uintptr_t)left | (uintptr_t)right | (uintptr_t)out6) & 3) {
    return SN_ERR_ARG;
  }
  const long total = 6L * h_px * (w >> 2);
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(k_pre_nv12, dim3(blocks), dim3(256), 0, st, dl, dr, w, w, h_px, dout);
  HIP_TRY(h, hipGetLastError());
  if (mem == SN_MEM_HOST)
    HIP_TRY(h, hipMemcpyAsync(out6, dout, (size_t)6 * w * h_px, hipMemcpyDeviceToHost, st));
  if (mem == SN_MEM_HOST || !stream) HIP_TRY(h, hipStreamSynchronize(st));
  return SN_OK;
}

int sn_infer_sbs_nv12(sn_handle* h, const uint8_t* sbs, int w2, int h_px, int32_t* out_i32, float* out_disp,
                      int8_t* out_tensor, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  // geometry check of FeedImg (stereonet_node.cpp:682-690): height == model h, width == 2 * model w
  if (!sbs || (!out_i32 && !out_disp) || !pre_args_ok(h, w2 / 2, h_px) || (w2 & 7) || (h_px & 1) ||
      (mem != SN_MEM_HOST && mem != SN_MEM_DEVICE)) {
    set_err(h, "sn_infer_sbs_nv12: image size does not match the model input");
    return SN_ERR_ARG;
  }
  int rc = check_device(h);
  if (rc) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  const int w = w2 / 2;
  const size_t HW = (size_t)h->H * h->W;
  const uint8_t* dsrc = sbs;
  if (mem == SN_MEM_HOST) {
    HIP_TRY(h, hipMemcpyAsync(h->ws.nv12, sbs, HW * 3, hipMemcpyHostToDevice, st));
    dsrc = h->ws.nv12;
  } else if ((uintptr_t)sbs & 3) {
    return SN_ERR_ARG;
  }
  int8_t* din = (mem == SN_MEM_DEVICE && out_tensor) ? out_tensor : h->ws.in6;
  const long total = 6L * h_px * (w >> 2);
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(k_pre_nv12, dim3(blocks), dim3(256), 0, st, dsrc, dsrc + w, w2, w, h_px, din);
  HIP_TRY(h, hipGetLastError());
  int32_t* draw = out_i32;
  float* ddisp = out_disp;
  if (mem == SN_MEM_HOST) {
    draw = out_i32 ? h->ws.out_raw : nullptr;
    ddisp = out_disp ? h->ws.out_disp : nullptr;
  }
  auto post = [&]() -> int {
    if (mem == SN_MEM_HOST) {
      if (out_i32) HIP_TRY(h, hipMemcpyAsync(out_i32, draw, HW * 4, hipMemcpyDeviceToHost, st));
      if (out_disp) HIP_TRY(h, hipMemcpyAsync(out_disp, ddisp, HW * 4, hipMemcpyDeviceToHost, st));
      if (out_tensor) HIP_TRY(h, hipMemcpyAsync(out_tensor, din, HW * 6, hipMemcpyDeviceToHost, st));
    }
    return SN_OK;
  };
  return run_forward(h, st, 1, din, ddisp, draw, true, mem == SN_MEM_HOST || !stream, post);
}

// FeedImg's split + CvtNV12Data2Tensors for a batch of side-by-side frames (device or host buffers): n frames of
// 3*H*W bytes -> n int8 model tensors of 6*H*W bytes.  The streaming ingest of bench.py --stream: the host ships the
// 2.76 MB camera frame instead of the 5.53 MB tensor.
int sn_preprocess_sbs_nv12_batch(sn_handle* h, int n, const uint8_t* sbs, int w2, int h_px, int8_t* out6, int mem,
                                 void* stream) {
  if (!h) return SN_ERR_ARG;
  if (!sbs || !out6 || n <= 0 || !pre_args_ok(h, w2 / 2, h_px) || (w2 & 7) || (h_px & 1) ||
      (mem != SN_MEM_HOST && mem != SN_MEM_DEVICE) || (mem == SN_MEM_HOST && n > h->max_batch)) {
    set_err(h, "sn_preprocess_sbs_nv12_batch: bad arguments");
    return SN_ERR_ARG;
  }
  if (mem == SN_MEM_DEVICE && (((uintptr_t)sbs | (uintptr_t)out6) & 3)) return SN_ERR_ARG;
  int rc = check_device(h);
  if (rc) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  const int w = w2 / 2;
  const size_t HW = (size_t)h->H * h->W;
  const long total = 6L * h_px * (w >> 2);
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  for (int i = 0; i < n; ++i) {
    const uint8_t* src = sbs + (size_t)i * 3 * HW;
    int8_t* dst = out6 + (size_t)i * 6 * HW;
    if (mem == SN_MEM_HOST) {           // one frame at a time through the NV12 staging buffer
      HIP_TRY(h, hipMemcpyAsync(h->ws.nv12, src, 3 * HW, hipMemcpyHostToDevice, st));
      src = h->ws.nv12;
      dst = h->ws.in6 + (size_t)i * 6 * HW;
    }
    hipLaunchKernelGGL(k_pre_nv12, dim3(blocks), dim3(256), 0, st, src, src + w, w2, w, h_px, dst);
  }
  HIP_TRY(h, hipGetLastError());
  if (mem == SN_MEM_HOST) HIP_TRY(h, hipMemcpyAsync(out6, h->ws.in6, (size_t)n * 6 * HW, hipMemcpyDeviceToHost, st));
  if (mem == SN_MEM_HOST || !stream) HIP_TRY(h, hipStreamSynchronize(st));
  return SN_OK;
}

// ---- async task slots (DnnNode::Run with is_sync_mode = false) ---------------------------------------
static int ensure_slots(sn_handle* h) {
  if (!h->slots.empty()) return SN_OK;
  const size_t HW = (size_t)h->H * h->W;
  h->slots.resize(h->task_num);
  for (auto& s : h->slots) {
    HIP_TRY(h, hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    HIP_TRY(h, hipEventCreate(&s.ev0));
    HIP_TRY(h, hipEventCreate(&s.ev1));
    int rc = alloc_ws(h, &s.ws, 1, 1, 1, 1);
    if (rc) return rc;
    HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&s.pin_in), 6 * HW, hipHostMallocDefault));
    HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&s.pin_raw), 4 * HW, hipHostMallocDefault));
    HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&s.pin_disp), 4 * HW, hipHostMallocDefault));
  }
  return SN_OK;
}

// kind 0: `in` is the int8 model tensor (6*H*W bytes); kind 1: the raw 2W x H side-by-side NV12 frame of FeedImg
// (3*H*W bytes: half the H2D traffic; split + chroma replication + ^0x80 run on the GPU in k_pre_nv12)
static int submit_common(sn_handle* h, const void* in, int kind, int32_t* out_i32, float* out_disp, int timeout_ms,
                         uint64_t* ticket) {
  if (!h || !in || (!out_i32 && !out_disp) || !ticket) return SN_ERR_ARG;
  std::unique_lock<std::mutex> lk(h->mu);
  int rc = check_device(h);
  if (rc) return rc;
  if ((rc = ensure_slots(h))) return rc;
  Slot* s = nullptr;
  auto find_free = [&]() {
    for (auto& c : h->slots)
      if (c.ticket == 0) {
        s = &c;
        return true;
      }
    return false;
  };
  if (timeout_ms < 0) {
    h->cv.wait(lk, find_free);
  } else if (!h->cv.wait_for(lk, std::chrono::milliseconds(timeout_ms), find_free)) {
    return SN_ERR_BUSY;
  }
  const size_t HW = (size_t)h->H * h->W;
  s->ticket = h->next_ticket++;
  s->user_raw = out_i32;
  s->user_disp = out_disp;
  // Every error exit below must hand the slot back (a slot left busy would make a later submit with
  // timeout -1 — what the node passes — block forever); *ticket is written on success only.
  struct SlotGuard {
    sn_handle* h;
    Slot* s;
    bool armed = true;
    ~SlotGuard() {
      if (!armed) return;
      s->ticket = 0;            // h->mu is still held by the caller's unique_lock
      h->cv.notify_one();
    }
  } guard{h, s};
  memcpy(s->pin_in, in, (kind == 1 ? 3 : 6) * HW);   // the caller may release its buffer as soon as we return
  const int mask = (out_i32 ? 1 : 0) | (out_disp ? 2 : 0);
  // arithmetic of this request: an SN_PREC_AUTO handle's current one (sn_wait folds the request's statistic in and repeats
  // a request that left the fp16 tower's envelope)
  const int mode = h->precision == SN_PREC_AUTO ? h->actl.st.mode : h->precision;
  // A streamed tower launch is one 160 KB-LDS workgroup per CU: while it runs nothing of another request fits the chip, so
  // requests in flight together simply queue (four in flight: the sum of their kernel times).  A request submitted while
  // others are in flight therefore leaves an eighth of the CUs to them: their low-resolution launches (tens of workgroups,
  // latency bound) run beside its tower — 2015-2030 -> 2135 pairs/s with four in flight (profiles/r06_async_wgs.txt), at
  // +14 % tower time for that request; a request that finds the GPU idle keeps every CU (latency of a lone frame unchanged).
  int others = 0;
  for (auto& c : h->slots)
    if (&c != s && c.ticket != 0) ++others;
  const int shared = (others > 0 && switches().async_share) ? 1 : 0;
  s->ws.tower_cu = shared ? h->num_cu * 7 / 8 : 0;
  const int mi = (mode == SN_PREC_F16X3 ? 0 : 2) + shared;
  s->mode_run = mode;
  auto enqueue = [&]() -> int {
    if (kind == 1) {
      HIP_TRY(h, hipMemcpyAsync(s->ws.nv12, s->pin_in, 3 * HW, hipMemcpyHostToDevice, s->stream));
      const long total = 6L * h->H * (h->W >> 2);
      const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
      hipLaunchKernelGGL(k_pre_nv12, dim3(blocks), dim3(256), 0, s->stream, s->ws.nv12, s->ws.nv12 + h->W, 2 * h->W, h->W,
                         h->H, s->ws.in6);
      HIP_TRY(h, hipGetLastError());
    } else {
      HIP_TRY(h, hipMemcpyAsync(s->ws.in6, s->pin_in, 6 * HW, hipMemcpyHostToDevice, s->stream));
    }
    const bool prof = h->profiling;
    h->profiling = false;   // stage events belong to the synchronous path
    const int r = forward(h, s->ws, s->stream, 1, s->ws.in6, out_disp ? s->ws.out_disp : nullptr,
                          out_i32 ? s->ws.out_raw : nullptr, false, mode);
    h->profiling = prof;
    if (r) return r;
    if (out_i32) HIP_TRY(h, hipMemcpyAsync(s->pin_raw, s->ws.out_raw, 4 * HW, hipMemcpyDeviceToHost, s->stream));
    if (out_disp) HIP_TRY(h, hipMemcpyAsync(s->pin_disp, s->ws.out_disp, 4 * HW, hipMemcpyDeviceToHost, s->stream));
    return SN_OK;
  };
  if (h->use_graphs && !s->gexec[kind][mask][mi] && s->uses[kind][mask][mi] >= 1) {
    // capture on the second use (the first, un-captured run has done every one-time initialisation)
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
      const int r = enqueue();
      const hipError_t e = hipStreamEndCapture(s->stream, &graph);
      if (r == SN_OK && e == hipSuccess && graph &&
          hipGraphInstantiate(&s->gexec[kind][mask][mi], graph, nullptr, nullptr, 0) != hipSuccess)
        s->gexec[kind][mask][mi] = nullptr;
      if (graph) hipGraphDestroy(graph);
    }
    if (!s->gexec[kind][mask][mi]) {
      (void)hipGetLastError();
      h->use_graphs = false;          // capture unsupported here: keep issuing plain launches (same kernels)
    }
  }
  HIP_TRY(h, hipEventRecord(s->ev0, s->stream));
  if (s->gexec[kind][mask][mi]) {
    HIP_TRY(h, hipGraphLaunch(s->gexec[kind][mask][mi], s->stream));
  } else {
    rc = enqueue();
    if (rc) return rc;
    ++s->uses[kind][mask][mi];
  }
  HIP_TRY(h, hipEventRecord(s->ev1, s->stream));
  guard.armed = false;
  *ticket = s->ticket;
  return SN_OK;
}

int sn_submit(sn_handle* h, const int8_t* in, int32_t* out_i32, float* out_disp, int timeout_ms,
              uint64_t* ticket) {
  return submit_common(h, in, 0, out_i32, out_disp, timeout_ms, ticket);
}

int sn_submit_nv12(sn_handle* h, const uint8_t* sbs, int w2, int h_px, int32_t* out_i32, float* out_disp,
                   int timeout_ms, uint64_t* ticket) {
  if (!h) return SN_ERR_ARG;
  // geometry check of FeedImg (stereonet_node.cpp:682-690): height == model h, width == 2 * model w
  if (!pre_args_ok(h, w2 / 2, h_px) || (w2 & 7) || (h_px & 1)) {
    set_err(h, "sn_submit_nv12: image size does not match the model input");
    return SN_ERR_ARG;
  }
  return submit_common(h, sbs, 1, out_i32, out_disp, timeout_ms, ticket);
}

int sn_wait(sn_handle* h, uint64_t ticket, float* infer_ms) {
  if (!h || ticket == 0) return SN_ERR_ARG;
  Slot* s = nullptr;
  {
    std::lock_guard<std::mutex> lk(h->mu);
    for (auto& c : h->slots)
      if (c.ticket == ticket) s = &c;
  }
  if (!s) return SN_ERR_TICKET;
  hipSetDevice(h->device);
  HIP_TRY(h, hipEventSynchronize(s->ev1));
  const size_t HW = (size_t)h->H * h->W;
  {
    // the request's refinement statistic; SN_PREC_AUTO: self-check on the first request, and a request that left the fp16
    // tower's envelope is repeated in SN_PREC_F16X3 on its own stream before its maps are handed over
    double lvl[kMaxLevels], res = 0.0;
    read_stats(h, s->ws, 1, lvl, &res);
    const bool is_auto = h->precision == SN_PREC_AUTO;
    int rc = SN_OK;
    if (is_auto && s->mode_run == SN_PREC_F16 && (rc = auto_selfcheck(h, s->ws, s->stream, s->ws.in6))) return rc;
    count_call(h, 1);
    const int next = fold_stats(h, lvl, res, 1, s->mode_run);
    if (is_auto && s->mode_run == SN_PREC_F16 && next == SN_PREC_F16X3) {
      if ((rc = forward(h, s->ws, s->stream, 1, s->ws.in6, s->user_disp ? s->ws.out_disp : nullptr,
                        s->user_raw ? s->ws.out_raw : nullptr, false, SN_PREC_F16X3)))
        return rc;
      if (s->user_raw) HIP_TRY(h, hipMemcpyAsync(s->pin_raw, s->ws.out_raw, 4 * HW, hipMemcpyDeviceToHost, s->stream));
      if (s->user_disp) HIP_TRY(h, hipMemcpyAsync(s->pin_disp, s->ws.out_disp, 4 * HW, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(h, hipEventRecord(s->ev1, s->stream));
      HIP_TRY(h, hipEventSynchronize(s->ev1));
      read_stats(h, s->ws, 1, lvl, &res);
      fold_stats(h, lvl, res, 1, SN_PREC_F16X3, false);
    }
  }
  if (s->user_raw) memcpy(s->user_raw, s->pin_raw, 4 * HW);
  if (s->user_disp) memcpy(s->user_disp, s->pin_disp, 4 * HW);
  if (infer_ms) {
    float ms = 0.f;
    HIP_TRY(h, hipEventElapsedTime(&ms, s->ev0, s->ev1));
    *infer_ms = ms;
  }
  {
    std::lock_guard<std::mutex> lk(h->mu);
    s->ticket = 0;
  }
  h->cv.notify_one();
  return SN_OK;
}

int sn_synchronize(sn_handle* h) {
  if (!h) return SN_ERR_ARG;
  int rc = check_device(h);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (auto& s : h->slots) HIP_TRY(h, hipStreamSynchronize(s.stream));
  return SN_OK;
}

// ---- measurement hooks ---------------------------------------------------------------------------------
int sn_set_profiling(sn_handle* h, int enable) {
  if (!h) return SN_ERR_ARG;
  h->profiling = enable != 0;
  return SN_OK;
}

int sn_get_stage_ms(sn_handle* h, float* ms, int count) {
  if (!h || !ms || count <= 0) return SN_ERR_ARG;
  for (int i = 0; i < count && i < SN_STAGE_COUNT; ++i) ms[i] = h->stage_ms[i];
  return SN_OK;
}

int sn_get_dominant_kernel(sn_handle* h, char* name, size_t cap, int* launches, double* flops, double* bytes) {
  if (!h) return SN_ERR_ARG;
  const int cur = h->precision == SN_PREC_AUTO ? h->actl.st.mode : h->precision;
  const bool f16 = cur == SN_PREC_F16;
  const double px = (double)h->Hp * h->Wp * chunk_pairs(h, h->ws, cur);
  if (f16 && h->fuse_mode == 4) {
    // the row-streaming fused residual block: SN_STAGE_DOMINANT times its launches of the first chunk one by one
    int n = 0;
    for (int i = 0; i < kNRefRes; ++i) {
      const bool last = i == kNRefRes - 1;
      if (stream_block_supports(kRefDil[i]) && !(last && h->tail_fuse)) ++n;
    }
    if (n > 0) {     // (n == 0, e.g. SN_STREAM_DIL=0: nothing is streamed — the per-layer description below applies)
      if (name && cap)
        snprintf(name, cap, "%s", "k_ref_block_stream_f16<DIL> (fused residual block: two 3x3 C->C convs + residual, fp16 MFMA 32x32x16)");
      if (launches) *launches = n;
      if (flops) *flops = 2.0 * (2.0 * px * kC * kC * 9);           // two convolutions per launch
      if (bytes) *bytes = px * kC * 2.0 * 2.0;                       // x read once + y written once; t never leaves LDS
      return SN_OK;
    }
  }
  if (cur == SN_PREC_F16X3) {
    int n = 0;
    for (int i = 0; i < kNRefRes; ++i)
      if (stream_x3_supports(kRefDil[i])) ++n;
    if (n > 0) {     // (SN_X3_STREAM=0: the per-layer description below applies)
      if (name && cap)
        snprintf(name, cap, "%s", "k_ref_block_stream_x3<DIL> (fused residual block: two 3x3 C->C convs + residual, 3 fp16 MFMAs 32x32x16 "
                                  "per product on hi/lo split operands; the FLOPs counted are the model's, not the three products')");
      if (launches) *launches = n;
      if (flops) *flops = 2.0 * (2.0 * px * kC * kC * 9);           // two convolutions per launch (algorithmic)
      if (bytes) *bytes = px * kC * 4.0 * 2.0;                       // x (hi + lo) read once + y written once; t never leaves LDS
      return SN_OK;
    }
  }
  if (name && cap)
    snprintf(name, cap, "%s",
             cur == SN_PREC_F16     ? "k_ref_conv_f16<DIL> (refinement 3x3 C->C, fp16 MFMA 32x32x16)"
             : cur == SN_PREC_F16X3 ? "k_ref_conv_f16x3<DIL> (refinement 3x3 C->C, 3x fp16 MFMA on hi/lo split operands)"
                                             : "k_ref_conv_f32<DIL> (refinement 3x3 C->C, weights-stationary, fp32 MFMA 32x32x2)");
  const int n_plain = kNRefRes, n_res = kNRefRes;      // per-layer forms: six launches without, six with a residual
  if (launches) *launches = n_plain + n_res;   // per refinement chunk
  if (flops) *flops = 2.0 * px * kC * kC * 9;
  // algorithmic HBM bytes per launch: read the 32-channel input once + write the output once, plus the
  // residual read on the launches that have one, averaged; element = 2 B (fp16) or 4 B (fp32)
  if (bytes) *bytes = px * kC * (f16 ? 2.0 : 4.0) * (2.0 * n_plain + 3.0 * n_res) / (double)(n_plain + n_res);
  return SN_OK;
}

// Parse's arithmetic per element (parser.cpp:84-86): the product f * B is a float, everything after it is double
__global__ __launch_bounds__(256) void k_depth_from_raw(const int32_t* __restrict__ raw, size_t n, float scale, float fB,
                                                        float* __restrict__ depth, float* __restrict__ disp) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float dis = (float)raw[i] * scale;
    depth[i] = (float)((double)fB / ((double)dis * 16.0 * 12.0) / 1000.0);
    if (disp) disp[i] = dis * 16.0f * 12.0f;
  }
}

int sn_depth_from_raw(sn_handle* h, int n, const int32_t* raw, float focal_px, float baseline_mm, float* depth_m, float* disp_px,
                      int mem, void* stream) {
  if (!h || !raw || !depth_m || n <= 0 || n > h->max_batch || (mem != SN_MEM_HOST && mem != SN_MEM_DEVICE)) return SN_ERR_ARG;
  int rc = check_device(h);
  if (rc) return rc;
  const size_t cnt = (size_t)n * h->H * h->W;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : h->stream;
  const float fB = focal_px * baseline_mm;      // float product, as in the reference expression
  const int32_t* draw = raw;
  float *ddepth = depth_m, *ddisp = disp_px;
  DevScope ds;
  if (mem == SN_MEM_HOST) {
    int32_t* a = nullptr;
    float *b = nullptr, *c = nullptr;
    HIP_TRY(h, ds.alloc(&a, cnt));
    HIP_TRY(h, ds.alloc(&b, cnt));
    if (disp_px) HIP_TRY(h, ds.alloc(&c, cnt));
    HIP_TRY(h, hipMemcpyAsync(a, raw, cnt * 4, hipMemcpyHostToDevice, st));
    draw = a;
    ddepth = b;
    ddisp = c;
  }
  unsigned grid = (unsigned)((cnt + 255) / 256);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(k_depth_from_raw, dim3(grid), dim3(256), 0, st, draw, cnt, kOutScale, fB, ddepth, ddisp);
  HIP_TRY(h, hipGetLastError());
  if (mem == SN_MEM_HOST) {
    HIP_TRY(h, hipMemcpyAsync(depth_m, ddepth, cnt * 4, hipMemcpyDeviceToHost, st));
    if (disp_px) HIP_TRY(h, hipMemcpyAsync(disp_px, ddisp, cnt * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
  }
  return SN_OK;
}

// Grows a buffer of the point-cloud state; a buffer is only ever replaced by a larger one, so a warm caller allocates nothing.
static hipError_t pc_grow(void** p, size_t* have, size_t bytes, bool pinned) {
  if (bytes <= *have) return hipSuccess;
  if (*p) {
    if (pinned) hipHostFree(*p);
    else hipFree(*p);
  }
  *p = nullptr;
  *have = 0;
  const hipError_t e = pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
  if (e == hipSuccess) *have = bytes;
  return e;
}

int sn_pointcloud_from_raw(sn_handle* h, int n, const int32_t* raw, const uint8_t* nv12, int nv12_pitch, const sn_camera* cam,
                           int layout, float* points, uint32_t* counts, int mem, void* stream) {
  if (!h || !raw || !cam || !points || n <= 0 || n > h->max_batch || ((uintptr_t)points & 15) ||
      (mem != SN_MEM_HOST && mem != SN_MEM_DEVICE) || (layout != SN_PC_ORGANISED && layout != SN_PC_COMPACT) ||
      (layout == SN_PC_COMPACT && !counts))
    return SN_ERR_ARG;
  if (!(cam->fx > 0.f) || !std::isfinite(cam->fx) || !(cam->fy > 0.f) || !std::isfinite(cam->fy) ||
      !(cam->baseline_mm > 0.f) || (cam->step != 1 && cam->step != 2 && cam->step != 4))
    return SN_ERR_ARG;
  if (nv12 && (nv12_pitch < h->W || (nv12_pitch & 1))) return SN_ERR_ARG;
  int rc = check_device(h);
  if (rc) return rc;
  auto& pc = h->pc;
  std::lock_guard<std::mutex> lk(pc.mu);
  if (!pc.stream) HIP_TRY(h, hipStreamCreateWithFlags(&pc.stream, hipStreamNonBlocking));
  if (!pc.ev) HIP_TRY(h, hipEventCreateWithFlags(&pc.ev, hipEventDisableTiming));
  const int W = h->W, H = h->H, step = cam->step;
  const int Wo = (W + step - 1) / step, Ho = (H + step - 1) / step;
  const int tiles = (Ho * Wo + kPcTile - 1) / kPcTile;
  const size_t raw_bytes = (size_t)n * H * W * 4, pts_bytes = (size_t)n * Ho * Wo * 16;
  const size_t frame = (size_t)nv12_pitch * (H + (H + 1) / 2);    // an odd height has ceil(H/2) chroma rows
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : pc.stream;
  HIP_TRY(h, hipStreamWaitEvent(st, pc.ev, 0));      // the previous call (any stream) is done with the scratch
  if (layout == SN_PC_COMPACT && (size_t)n * tiles * 4 > pc.scratch_bytes) {
    HIP_TRY(h, hipEventSynchronize(pc.ev));
    HIP_TRY(h, pc_grow(reinterpret_cast<void**>(&pc.scratch), &pc.scratch_bytes, (size_t)n * tiles * 4, false));
  }
  PcArgs a{raw, nv12, reinterpret_cast<float4*>(points), counts, pc.scratch, frame, W, H, Wo, Ho, step, nv12_pitch, tiles,
           kOutScale, cam->fx * cam->baseline_mm, cam->fx, cam->fy, cam->cx, cam->cy, cam->z_min_m, cam->z_max_m, 0};
  if (mem == SN_MEM_HOST) {
    HIP_TRY(h, pc_grow(&pc.pin[0], &pc.pin_bytes[0], raw_bytes, true));
    HIP_TRY(h, pc_grow(&pc.dev[0], &pc.dev_bytes[0], raw_bytes, false));
    HIP_TRY(h, pc_grow(&pc.dev[2], &pc.dev_bytes[2], pts_bytes, false));
    HIP_TRY(h, pc_grow(&pc.dev[3], &pc.dev_bytes[3], (size_t)n * 4, false));
    memcpy(pc.pin[0], raw, raw_bytes);
    HIP_TRY(h, hipMemcpyAsync(pc.dev[0], pc.pin[0], raw_bytes, hipMemcpyHostToDevice, st));
    if (nv12) {
      HIP_TRY(h, pc_grow(&pc.pin[1], &pc.pin_bytes[1], n * frame, true));
      HIP_TRY(h, pc_grow(&pc.dev[1], &pc.dev_bytes[1], n * frame, false));
      memcpy(pc.pin[1], nv12, n * frame);
      HIP_TRY(h, hipMemcpyAsync(pc.dev[1], pc.pin[1], n * frame, hipMemcpyHostToDevice, st));
      a.nv12 = static_cast<const uint8_t*>(pc.dev[1]);
    }
    a.raw = static_cast<const int32_t*>(pc.dev[0]);
    a.pts = static_cast<float4*>(pc.dev[2]);
    a.counts = counts ? static_cast<uint32_t*>(pc.dev[3]) : nullptr;
  }
  a.vec = step == 1 && (W & 3) == 0 && ((uintptr_t)a.raw & 15) == 0;
  if (layout == SN_PC_ORGANISED) {
    if (a.counts) HIP_TRY(h, hipMemsetAsync(a.counts, 0, (size_t)n * 4, st));
    const int nseg = Ho * ((Wo + 255) / 256);            // 256-column row segments, one per wave and iteration
    const int per_map = std::max(1, std::min((nseg + 3) / 4, 2048 / n));
    if (a.nv12) hipLaunchKernelGGL(k_pc_organised<true>, dim3(per_map, n), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_pc_organised<false>, dim3(per_map, n), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL(k_pc_count, dim3(tiles, n), dim3(256), 0, st, a);
    if (a.nv12) hipLaunchKernelGGL(k_pc_write<true>, dim3(tiles, n), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_pc_write<false>, dim3(tiles, n), dim3(256), 0, st, a);
  }
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipEventRecord(pc.ev, st));
  if (mem == SN_MEM_HOST) {
    if (counts) HIP_TRY(h, hipMemcpyAsync(counts, a.counts, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (layout == SN_PC_ORGANISED) {
      HIP_TRY(h, hipMemcpyAsync(points, a.pts, pts_bytes, hipMemcpyDeviceToHost, st));
    } else {
      HIP_TRY(h, hipStreamSynchronize(st));      // the counts say how much of every map to copy
      for (int k = 0; k < n; ++k)
        if (counts[k])
          HIP_TRY(h, hipMemcpyAsync(points + (size_t)k * Ho * Wo * 4, a.pts + (size_t)k * Ho * Wo, (size_t)counts[k] * 16,
                                    hipMemcpyDeviceToHost, st));
    }
  }
  if (mem == SN_MEM_HOST || !stream) HIP_TRY(h, hipStreamSynchronize(st));
  return SN_OK;
}

// ---- left-right consistency check (csrc/sn_lrcheck.hpp) --------------------------------------------------------------
static bool lrc_params_ok(const sn_lrc_params* p) {
  return p && std::isfinite(p->tau_px) && std::isfinite(p->tau_rel) && p->tau_px >= 0.f && p->tau_rel >= 0.f;
}

// buffer `which` of the handle's LrCheck state, at least `bytes` large (nullptr: the allocation failed)
static void* lrc_buf(sn_handle* h, int which, size_t bytes) {
  return pc_grow(&h->lrc.dev[which], &h->lrc.dev_bytes[which], bytes, false) == hipSuccess ? h->lrc.dev[which] : nullptr;
}
#define LRC_BUF(h, dst, type, which, bytes)                                     \
  do {                                                                          \
    if (!((dst) = static_cast<type>(lrc_buf(h, sn_handle::LrCheck::which, bytes)))) {   \
      set_err(h, "left-right check: out of device memory");                     \
      return SN_ERR_NOMEM;                                                      \
    }                                                                           \
  } while (0)

static int mirror_launch(sn_handle* h, hipStream_t st, int n, const int8_t* in, int8_t* out) {
  MirrorArgs a{in, out, n, h->H, h->W};
  const bool vec = (h->W & 15) == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
  const size_t items = (size_t)n * 6 * h->H * (vec ? h->W >> 4 : h->W);
  const unsigned grid = (unsigned)std::min<size_t>((items + 255) / 256, 8192);
  if (vec) hipLaunchKernelGGL(k_mirror_pair<true>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_mirror_pair<false>, dim3(grid), dim3(256), 0, st, a);
  HIP_TRY(h, hipGetLastError());
  return SN_OK;
}

// device pointers; right_out (nullable) receives the right map in right-image coordinates
static int lrc_launch(sn_handle* h, hipStream_t st, int n, const int32_t* left, const int32_t* right, const sn_lrc_params* p,
                      int32_t* out_raw, float* disp, uint8_t* mask, uint32_t* kept, int32_t* right_out) {
  LrcArgs a{left, right, out_raw, disp, mask, kept, right_out, h->W, h->H, (float)((double)kOutScale * kWireFactor),
            p->tau_px, p->tau_rel, p->right_mirrored != 0};
  const bool vec = (h->W & 3) == 0 &&
                   (((uintptr_t)left | (uintptr_t)right | (uintptr_t)out_raw | (uintptr_t)right_out) & 15) == 0 &&
                   ((uintptr_t)mask & 3) == 0;
  if (kept) HIP_TRY(h, hipMemsetAsync(kept, 0, (size_t)n * 4, st));
  const int nseg = h->H * ((h->W + 255) / 256);
  const int per_map = std::max(1, std::min((nseg + 3) / 4, 4096 / n));
  if (vec) hipLaunchKernelGGL(k_lr_check<true>, dim3(per_map, n), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_lr_check<false>, dim3(per_map, n), dim3(256), 0, st, a);
  HIP_TRY(h, hipGetLastError());
  return SN_OK;
}

int sn_mirror_pair_i8(sn_handle* h, int n, const int8_t* in, int8_t* out, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  const size_t bytes = (size_t)(n > 0 ? n : 0) * 6 * h->H * h->W;
  if (!in || !out || n <= 0 || n > h->max_batch || (mem != SN_MEM_HOST && mem != SN_MEM_DEVICE) ||
      ((uintptr_t)in < (uintptr_t)out + bytes && (uintptr_t)out < (uintptr_t)in + bytes)) {
    set_err(h, "sn_mirror_pair_i8: bad arguments");
    return SN_ERR_ARG;
  }
  int rc = check_device(h);
  if (rc) return rc;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : h->stream;
  const int8_t* din = in;
  int8_t* dout = out;
  if (mem == SN_MEM_HOST) {
    int8_t* stage;
    LRC_BUF(h, stage, int8_t*, kIn, bytes);
    LRC_BUF(h, dout, int8_t*, kMirror, bytes);
    HIP_TRY(h, hipMemcpyAsync(stage, in, bytes, hipMemcpyHostToDevice, st));
    din = stage;
  }
  if ((rc = mirror_launch(h, st, n, din, dout))) return rc;
  if (mem == SN_MEM_HOST) HIP_TRY(h, hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, st));
  if (mem == SN_MEM_HOST || !stream) HIP_TRY(h, hipStreamSynchronize(st));
  return SN_OK;
}

int sn_lr_check(sn_handle* h, int n, const int32_t* raw_left, const int32_t* raw_right, const sn_lrc_params* p,
                int32_t* out_raw, float* disp_inout, uint8_t* mask, uint32_t* kept, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  if (!raw_left || !raw_right || !lrc_params_ok(p) || (!out_raw && !mask) || n <= 0 || n > h->max_batch ||
      (mem != SN_MEM_HOST && mem != SN_MEM_DEVICE)) {
    set_err(h, "sn_lr_check: bad arguments");
    return SN_ERR_ARG;
  }
  int rc = check_device(h);
  if (rc) return rc;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : h->stream;
  const size_t cnt = (size_t)n * h->H * h->W;
  const int32_t *dl = raw_left, *dr = raw_right;
  int32_t* dout = out_raw;
  float* ddisp = disp_inout;
  uint8_t* dmask = mask;
  uint32_t* dkept = kept;
  if (mem == SN_MEM_HOST) {
    int32_t *l, *r;
    LRC_BUF(h, l, int32_t*, kLeft, cnt * 4);
    LRC_BUF(h, r, int32_t*, kRight, cnt * 4);
    HIP_TRY(h, hipMemcpyAsync(l, raw_left, cnt * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(r, raw_right, cnt * 4, hipMemcpyHostToDevice, st));
    dl = l;
    dr = r;
    dout = out_raw ? l : nullptr;            // masked in place
    if (disp_inout) {
      LRC_BUF(h, ddisp, float*, kDisp, cnt * 4);
      HIP_TRY(h, hipMemcpyAsync(ddisp, disp_inout, cnt * 4, hipMemcpyHostToDevice, st));
    }
    if (mask) LRC_BUF(h, dmask, uint8_t*, kMask, cnt);
    if (kept) LRC_BUF(h, dkept, uint32_t*, kKept, (size_t)n * 4);
  }
  if ((rc = lrc_launch(h, st, n, dl, dr, p, dout, ddisp, dmask, dkept, nullptr))) return rc;
  if (mem == SN_MEM_HOST) {
    if (out_raw) HIP_TRY(h, hipMemcpyAsync(out_raw, dout, cnt * 4, hipMemcpyDeviceToHost, st));
    if (disp_inout) HIP_TRY(h, hipMemcpyAsync(disp_inout, ddisp, cnt * 4, hipMemcpyDeviceToHost, st));
    if (mask) HIP_TRY(h, hipMemcpyAsync(mask, dmask, cnt, hipMemcpyDeviceToHost, st));
    if (kept) HIP_TRY(h, hipMemcpyAsync(kept, dkept, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  }
  if (mem == SN_MEM_HOST || !stream) HIP_TRY(h, hipStreamSynchronize(st));
  return SN_OK;
}

// L = forward(in), M = forward(mirror(in)), then the check of L against M in its mirrored storage: two run_forward calls, so
// each is counted, folded into the refinement statistic and (SN_PREC_AUTO, blocking) repeated by the usual rule.
int sn_infer_lrc(sn_handle* h, int n, const void* in, int in_kind, int w2, int h_px, const sn_lrc_params* p, int32_t* out_i32,
                 float* out_disp, int32_t* out_right_i32, uint8_t* mask, uint32_t* kept, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  if (!in || !lrc_params_ok(p) || (!out_i32 && !out_disp) || n <= 0 || n > h->max_batch ||
      (mem != SN_MEM_HOST && mem != SN_MEM_DEVICE) || (in_kind != SN_LRC_IN_TENSOR && in_kind != SN_LRC_IN_SBS_NV12)) {
    set_err(h, "sn_infer_lrc: bad arguments");
    return SN_ERR_ARG;
  }
  if (in_kind == SN_LRC_IN_SBS_NV12 && (!pre_args_ok(h, w2 / 2, h_px) || (w2 & 7) || (h_px & 1) ||
                                        (mem == SN_MEM_DEVICE && ((uintptr_t)in & 3)))) {
    set_err(h, "sn_infer_lrc: image size does not match the model input");
    return SN_ERR_ARG;
  }
  int rc = check_device(h);
  if (rc) return rc;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : h->stream;
  const bool host = mem == SN_MEM_HOST, blocking = host || !stream;
  const size_t HW = (size_t)h->H * h->W, cnt = (size_t)n * HW;
  const int8_t* din = static_cast<const int8_t*>(in);
  int8_t* dmir;
  int32_t *dleft = out_i32, *dsecond, *dright = out_right_i32;
  float* ddisp = out_disp;
  uint8_t* dmask = mask;
  uint32_t* dkept = kept;
  LRC_BUF(h, dmir, int8_t*, kMirror, cnt * 6);
  LRC_BUF(h, dsecond, int32_t*, kRight, cnt * 4);
  if (host || !out_i32) LRC_BUF(h, dleft, int32_t*, kLeft, cnt * 4);
  if (host) {
    if (out_disp) LRC_BUF(h, ddisp, float*, kDisp, cnt * 4);
    if (out_right_i32) LRC_BUF(h, dright, int32_t*, kRightOut, cnt * 4);
    if (mask) LRC_BUF(h, dmask, uint8_t*, kMask, cnt);
    if (kept) LRC_BUF(h, dkept, uint32_t*, kKept, (size_t)n * 4);
  }
  if (in_kind == SN_LRC_IN_SBS_NV12) {
    int8_t* ten;
    LRC_BUF(h, ten, int8_t*, kIn, cnt * 6);
    const int w = w2 / 2;
    const long total = 6L * h_px * (w >> 2);
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    for (int i = 0; i < n; ++i) {
      const uint8_t* src = static_cast<const uint8_t*>(in) + (size_t)i * 3 * HW;
      if (host) {                         // one frame at a time through the NV12 staging buffer
        HIP_TRY(h, hipMemcpyAsync(h->ws.nv12, src, 3 * HW, hipMemcpyHostToDevice, st));
        src = h->ws.nv12;
      }
      hipLaunchKernelGGL(k_pre_nv12, dim3(blocks), dim3(256), 0, st, src, src + w, w2, w, h_px, ten + (size_t)i * 6 * HW);
    }
    HIP_TRY(h, hipGetLastError());
    din = ten;
  } else if (host) {
    int8_t* ten;
    LRC_BUF(h, ten, int8_t*, kIn, cnt * 6);
    HIP_TRY(h, hipMemcpyAsync(ten, in, cnt * 6, hipMemcpyHostToDevice, st));
    din = ten;
  }
  auto nothing = []() -> int { return SN_OK; };
  if ((rc = run_forward(h, st, n, din, ddisp, dleft, n == 1, blocking, nothing))) return rc;
  if ((rc = mirror_launch(h, st, n, din, dmir))) return rc;
  if ((rc = run_forward(h, st, n, dmir, nullptr, dsecond, false, blocking, nothing))) return rc;
  sn_lrc_params q = *p;
  q.right_mirrored = 1;
  if ((rc = lrc_launch(h, st, n, dleft, dsecond, &q, dleft, ddisp, dmask, dkept, dright))) return rc;
  if (host) {
    if (out_i32) HIP_TRY(h, hipMemcpyAsync(out_i32, dleft, cnt * 4, hipMemcpyDeviceToHost, st));
    if (out_disp) HIP_TRY(h, hipMemcpyAsync(out_disp, ddisp, cnt * 4, hipMemcpyDeviceToHost, st));
    if (out_right_i32) HIP_TRY(h, hipMemcpyAsync(out_right_i32, dright, cnt * 4, hipMemcpyDeviceToHost, st));
    if (mask) HIP_TRY(h, hipMemcpyAsync(mask, dmask, cnt, hipMemcpyDeviceToHost, st));
    if (kept) HIP_TRY(h, hipMemcpyAsync(kept, dkept, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  }
  if (blocking) HIP_TRY(h, hipStreamSynchronize(st));
  return SN_OK;
}

// ---- confidence of the soft-argmin distribution and the mask on it (csrc/sn_confidence.hpp) ------------------------------------
static bool conf_params_ok(const sn_conf_params* p) {
  return p && std::isfinite(p->min_conf) && p->min_conf >= 0.f && p->min_conf <= 1.f;
}

// device pointers.  low: conf_in is a low-resolution plane [n][hl][wl] (upsampled, out_conf nullable); else a full-resolution
// map.  p == nullptr: no masking (out_conf only)
static int conf_launch(sn_handle* h, hipStream_t st, int n, bool low, const float* conf_in, const int32_t* raw,
                       const sn_conf_params* p, float* out_conf, int32_t* out_raw, float* disp, uint8_t* mask, uint32_t* kept) {
  if (!p && !(low && out_conf)) return SN_OK;      // nothing to write
  ConfArgs a{conf_in, raw, out_conf, out_raw, disp, mask, kept, h->hl, h->wl, h->H, h->W, p ? p->min_conf : 0.f, p != nullptr};
  if (p && kept) HIP_TRY(h, hipMemsetAsync(kept, 0, (size_t)n * 4, st));
  const int blocks = (int)(((size_t)h->H * h->W + 255) / 256);      // about 1024 workgroups per call: see k_conf_apply
  const dim3 grid((unsigned)std::max(1, std::min(blocks, 1024 / n)), (unsigned)n);
  if (low) hipLaunchKernelGGL(k_conf_apply<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_conf_apply<false>, grid, dim3(256), 0, st, a);
  HIP_TRY(h, hipGetLastError());
  return SN_OK;
}

// One forward pass whose soft-argmin epilogue also writes the confidence plane; the upsample + mask kernel is run_forward's
// `post`, so a call that SN_PREC_AUTO repeats in SN_PREC_F16X3 masks the repeated maps.
int sn_infer_conf(sn_handle* h, int n, const void* in, int in_kind, int w2, int h_px, const sn_conf_params* p, int32_t* out_i32,
                  float* out_disp, float* out_conf, uint8_t* mask, uint32_t* kept, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  if (!in || (p && !conf_params_ok(p)) || (!p && (mask || kept)) || (!out_i32 && !out_disp) || n <= 0 || n > h->max_batch ||
      (mem != SN_MEM_HOST && mem != SN_MEM_DEVICE) || (in_kind != SN_LRC_IN_TENSOR && in_kind != SN_LRC_IN_SBS_NV12)) {
    set_err(h, "sn_infer_conf: bad arguments");
    return SN_ERR_ARG;
  }
  if (in_kind == SN_LRC_IN_SBS_NV12 && (!pre_args_ok(h, w2 / 2, h_px) || (w2 & 7) || (h_px & 1) ||
                                        (mem == SN_MEM_DEVICE && ((uintptr_t)in & 3)))) {
    set_err(h, "sn_infer_conf: image size does not match the model input");
    return SN_ERR_ARG;
  }
  int rc = check_device(h);
  if (rc) return rc;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : h->stream;
  const bool host = mem == SN_MEM_HOST, blocking = host || !stream;
  const size_t HW = (size_t)h->H * h->W, cnt = (size_t)n * HW;
  const int8_t* din = static_cast<const int8_t*>(in);
  int32_t* draw = out_i32;
  float *ddisp = out_disp, *dconf = out_conf;
  uint8_t* dmask = mask;
  uint32_t* dkept = kept;
  if ((host && out_i32) || (p && !out_i32)) LRC_BUF(h, draw, int32_t*, kLeft, cnt * 4);      // the mask rules read the map
  if (host) {
    if (out_disp) LRC_BUF(h, ddisp, float*, kDisp, cnt * 4);
    if (out_conf) LRC_BUF(h, dconf, float*, kConf, cnt * 4);
    if (mask) LRC_BUF(h, dmask, uint8_t*, kMask, cnt);
    if (kept) LRC_BUF(h, dkept, uint32_t*, kKept, (size_t)n * 4);
  }
  if (in_kind == SN_LRC_IN_SBS_NV12) {
    int8_t* ten;
    LRC_BUF(h, ten, int8_t*, kIn, cnt * 6);
    const int w = w2 / 2;
    const long total = 6L * h_px * (w >> 2);
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    for (int i = 0; i < n; ++i) {
      const uint8_t* src = static_cast<const uint8_t*>(in) + (size_t)i * 3 * HW;
      if (host) {                         // one frame at a time through the NV12 staging buffer
        HIP_TRY(h, hipMemcpyAsync(h->ws.nv12, src, 3 * HW, hipMemcpyHostToDevice, st));
        src = h->ws.nv12;
      }
      hipLaunchKernelGGL(k_pre_nv12, dim3(blocks), dim3(256), 0, st, src, src + w, w2, w, h_px, ten + (size_t)i * 6 * HW);
    }
    HIP_TRY(h, hipGetLastError());
    din = ten;
  } else if (host) {
    int8_t* ten;
    LRC_BUF(h, ten, int8_t*, kIn, cnt * 6);
    HIP_TRY(h, hipMemcpyAsync(ten, in, cnt * 6, hipMemcpyHostToDevice, st));
    din = ten;
  }
  auto post = [&]() -> int {
    const int prc = conf_launch(h, st, n, true, h->ws.conf_low, draw, p, dconf, draw, ddisp, dmask, dkept);
    if (prc) return prc;
    if (host) {
      if (out_i32) HIP_TRY(h, hipMemcpyAsync(out_i32, draw, cnt * 4, hipMemcpyDeviceToHost, st));
      if (out_disp) HIP_TRY(h, hipMemcpyAsync(out_disp, ddisp, cnt * 4, hipMemcpyDeviceToHost, st));
      if (out_conf) HIP_TRY(h, hipMemcpyAsync(out_conf, dconf, cnt * 4, hipMemcpyDeviceToHost, st));
      if (mask) HIP_TRY(h, hipMemcpyAsync(mask, dmask, cnt, hipMemcpyDeviceToHost, st));
      if (kept) HIP_TRY(h, hipMemcpyAsync(kept, dkept, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    }
    return SN_OK;
  };
  return run_forward(h, st, n, din, ddisp, draw, n == 1, blocking, post, true);
}

int sn_conf_mask(sn_handle* h, int n, const int32_t* raw, const float* conf, const sn_conf_params* p, int32_t* out_raw,
                 float* disp_inout, uint8_t* mask, uint32_t* kept, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  if (!raw || !conf || !conf_params_ok(p) || (!out_raw && !mask) || n <= 0 || n > h->max_batch ||
      (mem != SN_MEM_HOST && mem != SN_MEM_DEVICE)) {
    set_err(h, "sn_conf_mask: bad arguments");
    return SN_ERR_ARG;
  }
  const size_t cnt = (size_t)n * h->H * h->W;
  {      // conf is read by every pixel's thread: it must not be one of the outputs
    const uintptr_t lo[4] = {(uintptr_t)out_raw, (uintptr_t)disp_inout, (uintptr_t)mask, (uintptr_t)kept};
    const size_t len[4] = {cnt * 4, cnt * 4, cnt, (size_t)n * 4};
    const uintptr_t c = (uintptr_t)conf;
    for (int i = 0; i < 4; ++i)
      if (lo[i] && lo[i] < c + cnt * 4 && c < lo[i] + len[i]) {
        set_err(h, "sn_conf_mask: conf overlaps an output");
        return SN_ERR_ARG;
      }
  }
  int rc = check_device(h);
  if (rc) return rc;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : h->stream;
  const int32_t* draw = raw;
  const float* dconf = conf;
  int32_t* dout = out_raw;
  float* ddisp = disp_inout;
  uint8_t* dmask = mask;
  uint32_t* dkept = kept;
  if (mem == SN_MEM_HOST) {
    int32_t* r;
    float* c;
    LRC_BUF(h, r, int32_t*, kLeft, cnt * 4);
    LRC_BUF(h, c, float*, kConf, cnt * 4);
    HIP_TRY(h, hipMemcpyAsync(r, raw, cnt * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(c, conf, cnt * 4, hipMemcpyHostToDevice, st));
    draw = r;
    dconf = c;
    dout = out_raw ? r : nullptr;            // masked in place
    if (disp_inout) {
      LRC_BUF(h, ddisp, float*, kDisp, cnt * 4);
      HIP_TRY(h, hipMemcpyAsync(ddisp, disp_inout, cnt * 4, hipMemcpyHostToDevice, st));
    }
    if (mask) LRC_BUF(h, dmask, uint8_t*, kMask, cnt);
    if (kept) LRC_BUF(h, dkept, uint32_t*, kKept, (size_t)n * 4);
  }
  if ((rc = conf_launch(h, st, n, false, dconf, draw, p, nullptr, dout, ddisp, dmask, dkept))) return rc;
  if (mem == SN_MEM_HOST) {
    if (out_raw) HIP_TRY(h, hipMemcpyAsync(out_raw, dout, cnt * 4, hipMemcpyDeviceToHost, st));
    if (disp_inout) HIP_TRY(h, hipMemcpyAsync(disp_inout, ddisp, cnt * 4, hipMemcpyDeviceToHost, st));
    if (mask) HIP_TRY(h, hipMemcpyAsync(mask, dmask, cnt, hipMemcpyDeviceToHost, st));
    if (kept) HIP_TRY(h, hipMemcpyAsync(kept, dkept, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  }
  if (mem == SN_MEM_HOST || !stream) HIP_TRY(h, hipStreamSynchronize(st));
  return SN_OK;
}

// ---- speckle removal and hole filling (csrc/sn_dispfilter.hpp) ---------------------------------------------------------------
int sn_filter_raw(sn_handle* h, int n, const int32_t* raw, const sn_filter_params* p, int32_t* out_raw, float* disp_inout,
                  uint8_t* mask, uint32_t* counts, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  const size_t HW = (size_t)h->H * h->W;
  if (!raw || !p || (!out_raw && !mask) || n <= 0 || n > h->max_batch || (mem != SN_MEM_HOST && mem != SN_MEM_DEVICE) ||
      p->speckle_max_px < 0 || (size_t)p->speckle_max_px > HW || !std::isfinite(p->speckle_diff_px) ||
      p->speckle_diff_px < 0.f || p->fill_max_px < 0 || (p->speckle_max_px == 0 && p->fill_max_px == 0) || HW > 0x7fffffffu) {
    set_err(h, "sn_filter_raw: bad arguments");
    return SN_ERR_ARG;
  }
  const size_t cnt = (size_t)n * HW;
  {      // out_raw == raw is the one overlap the kernels are written for
    const uintptr_t lo[5] = {(uintptr_t)raw, (uintptr_t)out_raw, (uintptr_t)disp_inout, (uintptr_t)mask, (uintptr_t)counts};
    const size_t len[5] = {cnt * 4, cnt * 4, cnt * 4, cnt, (size_t)n * 12};
    for (int i = 0; i < 5; ++i)
      for (int j = i + 1; j < 5; ++j)
        if (lo[i] && lo[j] && !(i == 0 && j == 1 && lo[0] == lo[1]) && lo[i] < lo[j] + len[j] && lo[j] < lo[i] + len[i]) {
          set_err(h, "sn_filter_raw: overlapping buffers (only out_raw == raw is allowed)");
          return SN_ERR_ARG;
        }
  }
  int rc = check_device(h);
  if (rc) return rc;
  auto& f = h->flt;
  std::lock_guard<std::mutex> lk(f.mu);
  if (!f.stream) HIP_TRY(h, hipStreamCreateWithFlags(&f.stream, hipStreamNonBlocking));
  if (!f.ev) HIP_TRY(h, hipEventCreateWithFlags(&f.ev, hipEventDisableTiming));
  const int slice = std::min(h->max_batch, kFltSlice);
  if (p->speckle_max_px && !f.scratch && hipMalloc(reinterpret_cast<void**>(&f.scratch), (size_t)slice * HW * 8) != hipSuccess) {
    f.scratch = nullptr;
    set_err(h, "sn_filter_raw: out of device memory");
    return SN_ERR_NOMEM;
  }
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : f.stream;
  HIP_TRY(h, hipStreamWaitEvent(st, f.ev, 0));      // the previous call (any stream) is done with the scratch and the staging
  const float S = (float)((double)kOutScale * kWireFactor);
  const float q = floorf(p->speckle_diff_px / S);
  FltArgs a{raw, out_raw, disp_inout, mask, counts, f.scratch, f.scratch ? f.scratch + (size_t)slice * HW : nullptr, h->W, h->H,
            (h->W + kFltTW - 1) / kFltTW, (h->H + kFltTH - 1) / kFltTH, q >= 4294967296.f ? 4294967296ll : (long long)q,
            (uint32_t)p->speckle_max_px, p->fill_max_px, S};
  if (mem == SN_MEM_HOST) {
    using F = sn_handle::Filter;
    HIP_TRY(h, pc_grow(&f.dev[F::kRaw], &f.dev_bytes[F::kRaw], cnt * 4, false));
    HIP_TRY(h, hipMemcpyAsync(f.dev[F::kRaw], raw, cnt * 4, hipMemcpyHostToDevice, st));
    a.raw = static_cast<const int32_t*>(f.dev[F::kRaw]);
    a.out_raw = out_raw ? static_cast<int32_t*>(f.dev[F::kRaw]) : nullptr;      // filtered in place
    if (disp_inout) {
      HIP_TRY(h, pc_grow(&f.dev[F::kDisp], &f.dev_bytes[F::kDisp], cnt * 4, false));
      HIP_TRY(h, hipMemcpyAsync(f.dev[F::kDisp], disp_inout, cnt * 4, hipMemcpyHostToDevice, st));
      a.disp = static_cast<float*>(f.dev[F::kDisp]);
    }
    if (mask) {
      HIP_TRY(h, pc_grow(&f.dev[F::kMask], &f.dev_bytes[F::kMask], cnt, false));
      a.mask = static_cast<uint8_t*>(f.dev[F::kMask]);
    }
    if (counts) {
      HIP_TRY(h, pc_grow(&f.dev[F::kCounts], &f.dev_bytes[F::kCounts], (size_t)n * 12, false));
      a.counts = static_cast<uint32_t*>(f.dev[F::kCounts]);
    }
  }
  const FltArgs all = a;
  if (a.counts) HIP_TRY(h, hipMemsetAsync(a.counts, 0, (size_t)n * 12, st));
  const bool vec = (h->W & 3) == 0 && ((uintptr_t)a.mask & 3) == 0;
  const int pairs = (a.tiles_x - 1) * h->H + (a.tiles_y - 1) * h->W;
  for (int k0 = 0; k0 < n; k0 += slice) {      // the scratch holds `slice` maps: walk the batch on the stream
    const int m = std::min(slice, n - k0);
    const size_t off = (size_t)k0 * HW;
    a.raw = all.raw + off;
    a.out_raw = all.out_raw ? all.out_raw + off : nullptr;
    a.disp = all.disp ? all.disp + off : nullptr;
    a.mask = all.mask ? all.mask + off : nullptr;
    a.counts = all.counts ? all.counts + (size_t)k0 * 3 : nullptr;
    if (a.max_px) {
      hipLaunchKernelGGL(k_flt_label, dim3(a.tiles_x * a.tiles_y, m), dim3(256), 0, st, a);
      if (pairs) hipLaunchKernelGGL(k_flt_seam, dim3((pairs + 255) / 256, m), dim3(256), 0, st, a);
      hipLaunchKernelGGL(k_flt_flatten, dim3((unsigned)((HW + 255) / 256), m), dim3(256), 0, st, a);
    }
    const int per_map = std::max(1, std::min((h->H + 3) / 4, 4096 / m));
    if (vec) hipLaunchKernelGGL(k_flt_apply<true>, dim3(per_map, m), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_flt_apply<false>, dim3(per_map, m), dim3(256), 0, st, a);
  }
  HIP_TRY(h, hipGetLastError());
  if (mem == SN_MEM_HOST) {
    if (out_raw) HIP_TRY(h, hipMemcpyAsync(out_raw, all.out_raw, cnt * 4, hipMemcpyDeviceToHost, st));
    if (disp_inout) HIP_TRY(h, hipMemcpyAsync(disp_inout, all.disp, cnt * 4, hipMemcpyDeviceToHost, st));
    if (mask) HIP_TRY(h, hipMemcpyAsync(mask, all.mask, cnt, hipMemcpyDeviceToHost, st));
    if (counts) HIP_TRY(h, hipMemcpyAsync(counts, all.counts, (size_t)n * 12, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(h, hipEventRecord(f.ev, st));
  if (mem == SN_MEM_HOST || !stream) HIP_TRY(h, hipStreamSynchronize(st));
  return SN_OK;
}

}  // extern "C"
