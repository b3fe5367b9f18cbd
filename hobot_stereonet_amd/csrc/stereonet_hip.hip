// stereonet_hip.hip — the one translation unit of the engine of libstereonet_hip.so: the headers below, one concern each and
// included in order, then the engine's own part of the public C ABI (include/stereonet_hip.h): create / destroy, io info,
// SN_PREC_AUTO's state machine, infer, preprocess, submit / wait and the measurement hooks.  The entry points that follow the
// network — depth, point cloud, mirror, left-right check, confidence, filter, smoother, temporal filter, rectifier — and the host helpers they share with the ones
// here (entry preamble, NV12 launcher) are in sn_postproc.hpp.  DESIGN.md §6 has the source map.
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
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/stereonet_hip.h"
#include "sn_internal.h"
#include "sn_switches.hpp"      // the SN_* environment switches
#include "sn_kernels.hpp"       // device code (with sn_pointcloud.hpp, sn_lrcheck.hpp, sn_dispfilter.hpp, sn_confidence.hpp, sn_smooth.hpp, sn_temporal.hpp, sn_rectify.hpp, sn_jpeg.hpp, sn_render.hpp, sn_obstacles.hpp, sn_ground.hpp, sn_costmap.hpp, sn_elevation.hpp, sn_inflate.hpp, sn_navfn.hpp, sn_rollout.hpp)
#include "sn_pointcloud.hpp"
#include "sn_lrcheck.hpp"
#include "sn_dispfilter.hpp"
#include "sn_confidence.hpp"
#include "sn_smooth.hpp"
#include "sn_temporal.hpp"
#include "sn_rectify.hpp"
#include "sn_jpeg.hpp"
#include "sn_render.hpp"
#include "sn_obstacles.hpp"
#include "sn_ground.hpp"
#include "sn_costmap.hpp"
#include "sn_elevation.hpp"
#include "sn_inflate.hpp"
#include "sn_navfn.hpp"
#include "sn_rollout.hpp"
#include "sn_engine.hpp"        // handle, workspace and layer types, error and allocation helpers
#include "sn_weights.hpp"       // .snw reader, weight packing and upload
#include "sn_launch.hpp"        // kernel launchers and tensor geometry
#include "sn_forward.hpp"       // workspace allocation, forward pass, refinement statistic, SN_PREC_AUTO
#include "sn_postproc.hpp"      // shared host staging + the C ABI of depth, point cloud, left-right check, confidence, filter, smoother, temporal filter, rectifier, JPEG encoder, render, obstacles, ground, costmap, elevation map, inflation, navigation function, rollout
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
    case SN_ERR_RANGE: return "activations left the range of fp16 (65504): the maps are not valid; use SN_PREC_FP32 for this model";
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
  h->obstacle_rle = sw.obstacle_rle;
  h->inflate_waves = sw.inflate_waves;
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
    if ((rc = upload_head_split(h, bw.next(1, kC, 9), &T.rout))) return fail(rc);
  }
  if (bw.off != blob.size()) return fail(SN_ERR_FORMAT);

  if ((rc = alloc_ws(h, &h->ws, h->max_batch, h->refine_chunk, h->tower_streams, h->refine_chunk_x3)))
    return fail(rc == SN_ERR_DEVICE ? SN_ERR_NOMEM : rc);
  *out = h;
  return SN_OK;
}

int sn_destroy(sn_handle* h) {
  if (!h) return SN_ERR_ARG;
  if (h->temporal_live.load() > 0) {      // a live sn_temporal holds this handle: refused, nothing is freed
    set_err(h, "sn_destroy: the handle still has temporal filters (sn_temporal_destroy them first)");
    return SN_ERR_BUSY;
  }
  if (h->rectify_live.load() > 0) {
    set_err(h, "sn_destroy: the handle still has rectifiers (sn_rectify_destroy them first)");
    return SN_ERR_BUSY;
  }
  if (h->costmap_live.load() > 0) {
    set_err(h, "sn_destroy: the handle still has costmaps (sn_costmap_destroy them first)");
    return SN_ERR_BUSY;
  }
  if (h->elevation_live.load() > 0) {
    set_err(h, "sn_destroy: the handle still has elevation maps (sn_elevation_destroy them first)");
    return SN_ERR_BUSY;
  }
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
    if (T.rout.wsplit != T.rout.w) hipFree(T.rout.wsplit);
    hipFree(T.rout.w);
  }
  hipFree(h->dump);
  h->pc.destroy();
  h->flt.destroy();
  h->smo.destroy();
  h->jpg.destroy();
  h->rnd.destroy();
  h->obs.destroy();
  h->gnd.destroy();
  h->inf.destroy();
  h->nav.destroy();
  h->roll.destroy();
  for (GrowBuf& b : h->stage.buf) b.release();
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
// px of the 2^k-weighted sum — a coarse level's error is upsampled with its map).  The self-check lowers this prior to the
// model's own slope where that is steeper (sn_auto_limit_px).
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
  // the self-check only TIGHTENS the limit: its slope is that of ONE pair, the first the handle saw in F16, and a later frame
  // may lose more per pixel of residual (tests/test_gpu_auto_sequences.py: a calm first frame, then a hard one)
  const double own = SN_AUTO_BUDGET_PX / s->epe_per_px;
  return own < s->envelope_px ? own : s->envelope_px;
}

int sn_auto_observe(sn_auto_state* s, double residual_px) {
  if (!s) return SN_ERR_ARG;
  // NaN / negative / +inf (a call the range check flagged): nothing the fp16 tower should be trusted with
  if (!(residual_px >= 0.0) || residual_px > kAutoResidualCap) residual_px = kAutoResidualCap;
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
  for (int lv = 0; lv < kMaxLevels; ++lv) out->nonfinite_px[lv] = a.last_range.level[lv];
  out->nonfinite_low_px = a.last_range.low;
  return SN_OK;
}

int sn_infer_batch(sn_handle* h, int n, const int8_t* in, int32_t* out_i32, float* out_disp, int mem,
                   void* stream) {
  if (!h) return SN_ERR_ARG;
  if (!in || (!out_i32 && !out_disp) || n <= 0 || n > h->max_batch) {
    set_err(h, "sn_infer_batch: bad arguments");
    return SN_ERR_ARG;
  }
  Call c;
  const int rc = enter(h, "sn_infer_batch", mem, stream, &h->stream, &c);
  if (rc) return rc;
  hipStream_t st = c.st;
  const size_t HW = (size_t)h->H * h->W;
  const int8_t* din = in;
  int32_t* draw = out_i32;
  float* ddisp = out_disp;
  if (c.host) {
    HIP_TRY(h, hipMemcpyAsync(h->ws.in6, in, (size_t)n * 6 * HW, hipMemcpyHostToDevice, st));
    din = h->ws.in6;
    draw = out_i32 ? h->ws.out_raw : nullptr;
    ddisp = out_disp ? h->ws.out_disp : nullptr;
  }
  auto post = [&]() -> int {
    if (c.host) {
      if (out_i32) HIP_TRY(h, hipMemcpyAsync(out_i32, draw, (size_t)n * HW * 4, hipMemcpyDeviceToHost, st));
      if (out_disp) HIP_TRY(h, hipMemcpyAsync(out_disp, ddisp, (size_t)n * HW * 4, hipMemcpyDeviceToHost, st));
    }
    return SN_OK;
  };
  return run_forward(h, st, n, din, ddisp, draw, n == 1, c.blocking, post);
}

int sn_infer_i8(sn_handle* h, const int8_t* in, int32_t* out_i32, float* out_disp, int mem, void* stream) {
  return sn_infer_batch(h, 1, in, out_i32, out_disp, mem, stream);
}

int sn_preprocess_nv12(sn_handle* h, const uint8_t* left, const uint8_t* right, int w, int h_px,
                       int8_t* out6, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  if (!left || !right || !out6 || w <= 0 || h_px <= 0 || (w & 3) || (h_px & 1) ||
      (size_t)w * h_px > (size_t)h->W * h->H) {
    set_err(h, "sn_preprocess_nv12: bad arguments");
    return SN_ERR_ARG;
  }
  Call c;
  const int rc = enter(h, "sn_preprocess_nv12", mem, stream, &h->stream, &c);
  if (rc) return rc;
  hipStream_t st = c.st;
  const size_t eye = (size_t)w * h_px * 3 / 2;
  const uint8_t *dl = left, *dr = right;
  int8_t* dout = out6;
  if (c.host) {
    HIP_TRY(h, hipMemcpyAsync(h->ws.nv12, left, eye, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(h->ws.nv12 + eye, right, eye, hipMemcpyHostToDevice, st));
    dl = h->ws.nv12;
    dr = h->ws.nv12 + eye;
    dout = h->ws.in6;
  } else if (((uintptr_t)left | (uintptr_t)right | (uintptr_t)out6) & 3) {
    return SN_ERR_ARG;
  }
  launch_pre_nv12(st, dl, dr, w, w, h_px, dout);
  HIP_TRY(h, hipGetLastError());
  if (c.host) HIP_TRY(h, hipMemcpyAsync(out6, dout, (size_t)6 * w * h_px, hipMemcpyDeviceToHost, st));
  if (c.blocking) HIP_TRY(h, hipStreamSynchronize(st));
  return SN_OK;
}

int sn_infer_sbs_nv12(sn_handle* h, const uint8_t* sbs, int w2, int h_px, int32_t* out_i32, float* out_disp,
                      int8_t* out_tensor, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  if (!sbs || (!out_i32 && !out_disp) || !sbs_frame_ok(h, w2, h_px)) {
    set_err(h, "sn_infer_sbs_nv12: image size does not match the model input");
    return SN_ERR_ARG;
  }
  Call c;
  const int rc = enter(h, "sn_infer_sbs_nv12", mem, stream, &h->stream, &c);
  if (rc) return rc;
  hipStream_t st = c.st;
  const size_t HW = (size_t)h->H * h->W;
  const uint8_t* dsrc = sbs;
  if (c.host) {
    HIP_TRY(h, hipMemcpyAsync(h->ws.nv12, sbs, HW * 3, hipMemcpyHostToDevice, st));
    dsrc = h->ws.nv12;
  } else if ((uintptr_t)sbs & 3) {
    return SN_ERR_ARG;
  }
  int8_t* din = (!c.host && out_tensor) ? out_tensor : h->ws.in6;
  launch_pre_nv12(st, dsrc, dsrc + w2 / 2, w2, w2 / 2, h_px, din);
  HIP_TRY(h, hipGetLastError());
  int32_t* draw = out_i32;
  float* ddisp = out_disp;
  if (c.host) {
    draw = out_i32 ? h->ws.out_raw : nullptr;
    ddisp = out_disp ? h->ws.out_disp : nullptr;
  }
  auto post = [&]() -> int {
    if (c.host) {
      if (out_i32) HIP_TRY(h, hipMemcpyAsync(out_i32, draw, HW * 4, hipMemcpyDeviceToHost, st));
      if (out_disp) HIP_TRY(h, hipMemcpyAsync(out_disp, ddisp, HW * 4, hipMemcpyDeviceToHost, st));
      if (out_tensor) HIP_TRY(h, hipMemcpyAsync(out_tensor, din, HW * 6, hipMemcpyDeviceToHost, st));
    }
    return SN_OK;
  };
  return run_forward(h, st, 1, din, ddisp, draw, true, c.blocking, post);
}

// FeedImg's split + CvtNV12Data2Tensors for a batch of side-by-side frames (device or host buffers): n frames of
// 3*H*W bytes -> n int8 model tensors of 6*H*W bytes.  The streaming ingest of bench.py --stream: the host ships the
// 2.76 MB camera frame instead of the 5.53 MB tensor.
int sn_preprocess_sbs_nv12_batch(sn_handle* h, int n, const uint8_t* sbs, int w2, int h_px, int8_t* out6, int mem,
                                 void* stream) {
  if (!h) return SN_ERR_ARG;
  if (!sbs || !out6 || n <= 0 || !sbs_frame_ok(h, w2, h_px) || (mem == SN_MEM_HOST && n > h->max_batch)) {
    set_err(h, "sn_preprocess_sbs_nv12_batch: bad arguments");
    return SN_ERR_ARG;
  }
  if (mem == SN_MEM_DEVICE && (((uintptr_t)sbs | (uintptr_t)out6) & 3)) return SN_ERR_ARG;
  Call c;
  int rc = enter(h, "sn_preprocess_sbs_nv12_batch", mem, stream, &h->stream, &c);
  if (rc) return rc;
  const size_t HW = (size_t)h->H * h->W;
  if ((rc = sbs_to_tensors(h, c.st, n, sbs, w2, h_px, c.host, c.host ? h->ws.in6 : out6))) return rc;
  if (c.host) HIP_TRY(h, hipMemcpyAsync(out6, h->ws.in6, (size_t)n * 6 * HW, hipMemcpyDeviceToHost, c.st));
  if (c.blocking) HIP_TRY(h, hipStreamSynchronize(c.st));
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

// Hands a busy slot back when it goes out of scope, unless disarmed: a slot left busy would make a later submit with
// timeout -1 — what the node passes — block forever.  take_mu: the owner does not hold h->mu.
struct SlotGuard {
  sn_handle* h;
  Slot* s;
  bool take_mu;
  bool armed = true;
  ~SlotGuard() {
    if (!armed) return;
    if (take_mu) h->mu.lock();
    s->ticket = 0;
    if (take_mu) h->mu.unlock();
    h->cv.notify_one();
  }
};

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
  // Every error exit below must hand the slot back; *ticket is written on success only.
  SlotGuard guard{h, s, false};           // h->mu is held by lk
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
      launch_pre_nv12(s->stream, s->ws.nv12, s->ws.nv12 + h->W, 2 * h->W, h->W, h->H, s->ws.in6);
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
    } else {
      ++h->graphs_instantiated;
    }
  }
  HIP_TRY(h, hipEventRecord(s->ev0, s->stream));
  if (s->gexec[kind][mask][mi]) {
    HIP_TRY(h, hipGraphLaunch(s->gexec[kind][mask][mi], s->stream));
    ++h->graph_launches;
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
  if (!sbs_frame_ok(h, w2, h_px)) {
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
  SlotGuard guard{h, s, true};       // every exit from here on consumes the ticket; an error exit writes no outputs
  hipSetDevice(h->device);
  HIP_TRY(h, hipEventSynchronize(s->ev1));
  const size_t HW = (size_t)h->H * h->W;
  // the request's refinement statistic; SN_PREC_AUTO: self-check on the first request, and a request that left the fp16
  // tower's envelope is repeated in SN_PREC_F16X3 on its own stream before its maps are handed over
  auto rerun = [&]() -> int {
    const int r = forward(h, s->ws, s->stream, 1, s->ws.in6, s->user_disp ? s->ws.out_disp : nullptr,
                          s->user_raw ? s->ws.out_raw : nullptr, false, SN_PREC_F16X3);
    if (r) return r;
    if (s->user_raw) HIP_TRY(h, hipMemcpyAsync(s->pin_raw, s->ws.out_raw, 4 * HW, hipMemcpyDeviceToHost, s->stream));
    if (s->user_disp) HIP_TRY(h, hipMemcpyAsync(s->pin_disp, s->ws.out_disp, 4 * HW, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(h, hipEventRecord(s->ev1, s->stream));
    HIP_TRY(h, hipEventSynchronize(s->ev1));
    return SN_OK;
  };
  const bool check = h->precision == SN_PREC_AUTO && s->mode_run == SN_PREC_F16;
  RangeCount range;          // of the arithmetic whose maps are handed over
  if (const int rc = settle(h, s->ws, s->stream, 1, s->ws.in6, s->mode_run, check, true, rerun, &range)) return rc;
  float ms = 0.f;
  if (infer_ms) HIP_TRY(h, hipEventElapsedTime(&ms, s->ev0, s->ev1));      // the last exit that leaves the outputs unwritten
  if (infer_ms) *infer_ms = ms;
  if (s->user_raw) memcpy(s->user_raw, s->pin_raw, 4 * HW);
  if (s->user_disp) memcpy(s->user_disp, s->pin_disp, 4 * HW);
  return range_result(h, range);         // SN_ERR_RANGE: the maps were copied and the ticket is consumed
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

}  // extern "C"
