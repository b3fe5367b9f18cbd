// sn_engine.hpp — the engine's data: layer, workspace, tower, async-slot and SN_PREC_AUTO types, the handle (sn_handle), and
// the helpers every other part uses (HIP_TRY, set_err, memset_now, GrowBuf, dalloc, DevScope, check_device).  No kernel is launched
// here.  Part of the single translation unit stereonet_hip.hip.
#pragma once

namespace {

using namespace sn;

constexpr int kNDown = 4, kNFeatRes = 6, kNAgg = 4, kNRefRes = 6;
constexpr int kRefDil[kNRefRes] = {1, 2, 4, 8, 1, 1};
constexpr float kOutScale = 2.60443857769133e-6f;   // stereonet_node.cpp:282
constexpr double kWireFactor = 16.0 * 12.0;         // parser.cpp:86
constexpr double kAutoEnvelopeSingle = 1.0, kAutoEnvelopeMulti = 2.9;   // sn_auto_envelope_px
constexpr double kAutoResidualCap = 1e30;     // what sn_auto_observe folds in for a residual that is NaN, negative or +inf
constexpr int kMaxPieceEvents = 64;
constexpr int kMaxTowerStreams = 2;

#define HIP_TRY(h, expr)                                                              \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) {                                                           \
      set_err(h, std::string(#expr) + ": " + hipGetErrorString(e_));                  \
      return SN_ERR_DEVICE;                                                           \
    }                                                                                 \
  } while (0)

// hipMemset runs on the legacy default stream and may return before the device has finished; the engine's streams are
// created hipStreamNonBlocking and do NOT order themselves behind it.  A kernel launched on one of them right after a
// plain hipMemset of its output can therefore be overtaken by the memset (seen once as a parity-hook flake in round 4:
// zeros in a freshly written tensor).  Every memset of a buffer that another stream touches next goes through this.
inline hipError_t memset_now(void* p, int v, size_t bytes) {
  hipError_t e = hipMemset(p, v, bytes);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(nullptr);
}

// A device (or pinned host) buffer that is only ever replaced by a larger one, so a warm caller allocates nothing.
struct GrowBuf {
  void* p = nullptr;
  size_t cap = 0;
  bool pinned = false;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    const hipError_t e = pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    else p = nullptr;
    return e;
  }
  void release() {
    if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
};

// A lane: what a post-processing stage owns so that it may run beside sn_submit / sn_wait and on any stream of the caller's.
// Slots names the buffers (an enum that ends in kCount).  Everything is created on first use; the call bracket that locks,
// orders and stages a call on a lane is LaneCall (sn_postproc.hpp).
template <class Slots>
struct Lane : Slots {
  std::mutex mu;
  hipStream_t stream = nullptr;      // the stage's own stream: a call without a stream of the caller's runs here
  hipEvent_t ev = nullptr;           // the last enqueue (on any stream) that used the buffers or the owner's state
  GrowBuf buf[Slots::kCount];
  void destroy() {
    if (stream) (void)hipStreamSynchronize(stream);
    if (ev) {
      (void)hipEventSynchronize(ev);      // a call that was only enqueued on a caller's stream
      (void)hipEventDestroy(ev);
    }
    if (stream) (void)hipStreamDestroy(stream);
    for (GrowBuf& b : buf) b.release();
    stream = nullptr, ev = nullptr;
  }
};

struct ConvLayer {
  uint4* wx3 = nullptr;    // device, split fp16 A-fragments [cin_pad/16][9][hi|lo][64 lanes] (fp16 modes, 3x3 layers)
  float* wpk = nullptr;    // device, packed [cin_pad][taps][32]
  float* bias = nullptr;   // device [32]
  int cin = 0, cin_pad = 0, taps = 0;
};

struct Down0F16 {           // first down-conv on the fp16 MFMA (k_down0_f16): 8 K-steps x (hi, lo) A-fragments
  uint4* wfrag = nullptr;   // device [8][2][64] slots
};

struct Down01W {            // down-convs 0 and 1 folded into one 13x13 stride-4 conv (sn_down01.hpp): nine weight classes
  uint4* wfrag = nullptr;   // device [9][39][2][64] slots
  float* bias = nullptr;    // device [9][32]
};

struct RefLayerF16 {        // fp16 tower layer: 18 MFMA A-fragments + fp32 bias
  uint4* wfrag = nullptr;   // device [9][2][64] slots
  float* bias = nullptr;
};

struct HeadLayer {          // C -> 1 layers (VALU kernels)
  float* w = nullptr;       // device [32][taps]
  float bias = 0.f;
  // ref*.out, fp16 modes (upload_head_split): the head kernels split w into a hi / lo pair of fp16 in registers, and fp16 has
  // no normal numbers below 2^-14 — a head whose weights are small (a tower that works at large activations) would lose them
  // there.  wsplit = w * 2^e with e chosen at load, biassplit = bias * 2^e, unscale = 2^-e: the kernels get (wsplit, biassplit,
  // dmax * unscale), so that dmax * (bias + sum) is the same number with every power of two exact.  e = 0 (wsplit == w)
  // unless the largest |w| is below 2^-12.
  float* wsplit = nullptr;
  float biassplit = 0.f, unscale = 1.f;
  uint4* pfrag = nullptr;   // agg.out only, fp16 modes: split A fragments of the taps-as-M contraction [2][hi|lo][64] (k_agg_x3s_dma HEADP)
};

constexpr int kMaxLevels = 4, kMultiLevels = 4;              // hierarchical refinement: 1/8, 1/4, 1/2, 1
constexpr int kStatWords = 8;                                // refinement statistic: [level 0..3] sum |D r|, [4] self-check sum |a - b|; each with its non-finite count in the same lines
constexpr size_t kStatU64 = (size_t)kStatWords * kStatWordStride;   // each word = kStatSlots partial sums in separate 128-byte lines
constexpr int kTileCtrStride = 8 * 16;                       // uints per tower launch (one 64-B line per XCD)
constexpr size_t kTileCtrBytes = (size_t)2 * 6 * kTileCtrStride * sizeof(unsigned);   // 2 * kNRefRes launches

struct Workspace {          // activations for up to `nb` pairs
  int nb = 0, rb = 0, pb = 0;   // batch capacity, pairs per tower launch, pairs per low-res piece
  int rb_x3 = 0;                // SN_PREC_AUTO: pairs per tower launch while the handle runs in SN_PREC_F16X3 (same buffers)
  int tower_cu = 0;             // > 0: workgroups of a streamed tower launch (an async slot that shares the GPU, submit_common)
  int rbk_x3[4] = {};           // ... and per coarse level
  // refinement statistic: one 64-bit fixed-point sum of |D r| per level (refine_stat_commit) + the self-check's sum at [4];
  // copied to the pinned twin at the end of every forward()
  unsigned long long* stats = nullptr;
  unsigned long long* stats_host = nullptr;
  int8_t* in6 = nullptr;
  float* down[3] = {nullptr, nullptr, nullptr};
  float* low[3] = {nullptr, nullptr, nullptr};
  float* feat = nullptr;
  float* vol[2] = {nullptr, nullptr};
  uint4* volp[2] = {nullptr, nullptr};
  uint4* lowp[2] = {nullptr, nullptr};            // zero-bordered (x, t) of the 3x3 feature layers (fp16 modes, FeatPad)
  uint4* downp[3] = {nullptr, nullptr, nullptr};   // zero-bordered inputs of down-convs 1..3 (fp16 modes, DownDma)   // zero-bordered split-slot volumes of the aggregation layers (fp16 modes, VolPad)
  float* cost = nullptr;     // [nb][Dl][hl][wl] (debug / parity)
  float* disp_low = nullptr;
  float* conf_low = nullptr; // [nb][hl][wl]: the soft-argmin's confidence plane (calls that ask for it: sn_infer_conf)
  int ns = 1;                 // tower streams this workspace serves: one (x, t) activation pair per stream
  float* ref[2 * kMaxTowerStreams] = {};
  uint4* ref16[2 * kMaxTowerStreams] = {};   // fp16 NCHW8c padded (fp16 modes): [2 * stream + {x, t}]
  uint4* ref16_raw[2 * kMaxTowerStreams] = {};            // the allocations behind them (alloc_ref16)
  // hierarchical refinement, levels 1..: the coarse levels run once per low-resolution PIECE (pb pairs), in chunks
  // of rbk[level] = min(pb, rb * 4^level) pairs (the same activation footprint per launch as level 0).  Activation
  // pairs (their own zero borders) for rbk pairs; image pyramid [pb][3][Hk][Wk] and level maps [pb][Hk][Wk].
  int rbk[kMaxLevels] = {};
  float* ref_lv[kMaxLevels][2] = {};
  uint4* ref16_lv[kMaxLevels][2] = {};
  uint4* ref16_lv_raw[kMaxLevels][2] = {};
  float* pyr[kMaxLevels] = {};
  float* lvl_disp[kMaxLevels] = {};
  int n_chunks = 0;
  unsigned* tile_ctr = nullptr;           // dynamic tile queues of the fp16 tower: [12 launches][8 XCDs][16] uints
  float* out_disp = nullptr;
  int32_t* out_raw = nullptr;
  uint8_t* nv12 = nullptr;   // staging for NV12 inputs (2 eyes or one side-by-side frame)
};

struct Tower {               // one refinement level: weights (in the forms the precision mode needs) + geometry
  ConvLayer rin, rres[kNRefRes][2];
  Down0F16 refin;
  RefLayerF16 rres16[kNRefRes][2];      // SN_PREC_F16 (and AUTO): plain fp16 A fragments
  RefLayerF16 rres16x3[kNRefRes][2];    // SN_PREC_F16X3 (and AUTO): hi / lo split A fragments
  HeadLayer rout;
  RefGeom rg{};
  int Hk = 0, Wk = 0;        // padded size of this level: Hp >> k, Wp >> k
};

struct Slot {                // async request slot (sn_submit / sn_wait)
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  Workspace ws;
  int8_t* pin_in = nullptr;
  int32_t* pin_raw = nullptr;
  float* pin_disp = nullptr;
  int32_t* user_raw = nullptr;
  float* user_disp = nullptr;
  uint64_t ticket = 0;       // 0 = free
  // hipGraph of {H2D, forward, D2H} per output mask (1 = int32, 2 = float, 3 = both): the second request with a
  // given mask is captured, later ones replay it (the ~45 launches of a single-pair forward are launch-bound)
  // the first index is the input kind: 0 = int8 model tensor (sn_submit), 1 = side-by-side NV12 frame (sn_submit_nv12)
  // the last index is the arithmetic the request runs in (0 = SN_PREC_F16X3, 1 = anything else): SN_PREC_AUTO may change it
  hipGraphExec_t gexec[2][4][4] = {};       // [input kind][output mask][arithmetic x (alone | sharing the GPU)]
  int uses[2][4][4] = {};
  int mode_run = 0;          // arithmetic of the request in flight (SN_PREC_*)
};

// SN_PREC_AUTO (include/stereonet_hip.h): the handle starts in SN_PREC_F16 and moves to SN_PREC_F16X3 when the refinement
// statistic leaves the envelope inside which the fp16 tower keeps EPE <= 1e-3 px, or when the self-check says so.
// The range check of one call (SN_ERR_RANGE, sn_kernels.hpp above stat_commit_line): non-finite pixels per refinement level
// and in the low-resolution branch's soft-argmin.
struct RangeCount {
  unsigned long long level[4] = {}, low = 0;
  bool any() const { return (level[0] | level[1] | level[2] | level[3] | low) != 0; }
};

struct AutoCtl {
  sn_auto_state st{};
  bool calibrated = false;       // the self-check (one pair in both arithmetics) has run since the handle last entered F16
  bool pending = false;          // a stream-enqueued call's statistic has not been folded in yet (ev_stats marks it)
  int pending_mode = 0, pending_n = 0;
  double selfcheck_epe = -1.0, selfcheck_res = -1.0;
  double last_level[4] = {}, last_res = 0.0;
  RangeCount last_range;         // the range check's counts of the same call
  int last_mode = 0;
  uint64_t calls = 0, pairs = 0, reruns = 0;
};

// What a persistent launcher launched: workgroups and work units (tiles; half tiles for k_ref_conv_f32; flat rows for the
// streamed blocks).  Optional out-parameter of the launchers (sn_launch.hpp), read by the parity hooks only.
struct LaunchInfo {
  int wgs = 0, units = 0;
};

}  // namespace

struct sn_handle {
  int device = 0;
  int W = 0, H = 0, D = 0, Wp = 0, Hp = 0, wl = 0, hl = 0, Dl = 0;
  int max_batch = 1, precision = SN_PREC_F16, task_num = 4, refine_chunk = 1, piece = 16;
  // `precision` is what the caller configured; SN_PREC_AUTO runs in actl.st.mode (SN_PREC_F16 or SN_PREC_F16X3)
  AutoCtl actl;
  std::mutex mu_cal;         // the self-check's scratch maps (chk) are shared by every slot
  float* chk[2] = {nullptr, nullptr};
  hipEvent_t ev_stats = nullptr;
  int refine_chunk_x3 = 1;   // SN_PREC_AUTO: pairs per tower launch in SN_PREC_F16X3
  hipStream_t stream = nullptr;
  // piece pipeline: the low-resolution branch of piece k+1 runs on s_low while the refinement towers of piece k run
  // on s_tow[]; consecutive tower chunks alternate between the tower streams so that the ramp-up / tail of one
  // chunk's launches is filled by the other chunk's workgroups
  hipStream_t s_low = nullptr, s_tow[kMaxTowerStreams] = {};
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_tow_join[kMaxTowerStreams] = {}, ev_piece[kMaxPieceEvents] = {};
  bool overlap = true;
  int tower_streams = kMaxTowerStreams;
#if SN_DIAGNOSTICS
  unsigned ablate_x = 0;     // SN_ABLATE_X mask (diagnostic build only): layers whose input tensor gets its lo slots zeroed
#else
  static constexpr unsigned ablate_x = 0;      // the shipping library has no ablation code: every test of it folds away
#endif
  bool obstacle_rle = true;  // sn_obstacles_from_raw accumulates run-length per lane; SN_OBSTACLE_RLE=0: one set of atomics per point
  int inflate_waves = 0;     // SN_INFLATE_WAVES: 4 or 16 waves per workgroup of k_inflate whatever the call's size; 0: by size (in_waves)
  bool tail_fuse = true;     // the streamed last block carries the head (tail form); SN_TAIL_FUSE=0: block + k_head_final_f16
  int fuse_mode = 4;         // SN_FUSE: 4 = streaming fused blocks (default), 0 = two launches per block
  unsigned* dump = nullptr;  // 2 KB device scratch: where lanes without an output pixel store (fused head)
  bool use_graphs = true;    // hipGraph replay for the async single-pair path (SN_NO_GRAPH disables)
  bool stream_prio = false;  // the pipeline streams were created with the device's highest priority (sn_create_prio)
  ConvLayer down[kNDown], fres[kNFeatRes][2], fout, agg[kNAgg];
  Down0F16 down0;
  Down01W down01;            // fp16 modes, unless SN_DOWN01=0
  bool fold_down01 = false;
  HeadLayer aout;
  // refinement towers: tw[0] = full resolution (the only one of a single-scale model); a hierarchical ("multi") model
  // has levels = kMultiLevels towers, tw[k] working at 1/2^k resolution
  int levels = 1;
  Tower tw[kMaxLevels];
  int num_cu = 256;
  // parity hooks only (sn_dbg_set_grid_cus, sn_dbg_last_launch): the CU count the sn_dbg_* hooks size their grids with
  // (0 = num_cu) and what the last swept launch reported.  The forward pass reads neither.
  int dbg_grid_cus = 0;
  LaunchInfo dbg_launch;
  Workspace ws;
  std::vector<Slot> slots;
  std::mutex mu;
  std::condition_variable cv;
  uint64_t next_ticket = 1;
  // what the slots did over the handle's life (submit_common, under mu; read by sn_dbg_slot_graphs): graphs instantiated and
  // requests served by hipGraphLaunch
  int graphs_instantiated = 0, graph_launches = 0;
  // profiling
  bool profiling = false;
  hipEvent_t ev[8] = {};
  hipEvent_t ev_dom[2 * 6] = {};   // profiling: one pair around every streamed block of the first chunk (the dominant kernel)
  int dom_pairs = 0;
  float stage_ms[SN_STAGE_COUNT] = {};
  mutable std::string err;
  mutable std::mutex err_mu;  // err is written by failing calls on any thread (sn_pointcloud_from_raw beside sn_wait)
  // The lanes of the handle's post-processing stages (Lane above): each may run beside sn_submit / sn_wait.
  // sn_pointcloud_from_raw.  compact form: valid samples per tile; host mode: raw, nv12, points, counts, and the pinned staging
  // of raw and nv12
  struct PointCloudSlots {
    enum { kScratch = 0, kRaw, kNv12, kPoints, kCounts, kPinRaw, kPinNv12, kCount };
  };
  struct PointCloud : Lane<PointCloudSlots> {
    PointCloud() { buf[kPinRaw].pinned = buf[kPinNv12].pinned = true; }
  } pc;
  // sn_filter_raw.  label[slice][H][W] then size[slice][H][W]; host mode: map (filtered in place), float map, mask, counts
  struct FilterSlots {
    enum { kScratch = 0, kRaw, kDisp, kMask, kCounts, kCount };
  };
  using Filter = Lane<FilterSlots>;
  Filter flt;
  // sn_smooth_raw.  the copy of a slice that an in-place call reads; host mode: map, guide, result, float map, mask, counts
  struct SmoothSlots {
    enum { kScratch = 0, kRaw, kGuide, kOut, kDisp, kMask, kCounts, kCount };
  };
  using Smooth = Lane<SmoothSlots>;
  Smooth smo;
  // sn_jpeg_encode_nv12.  the coefficients, the slices' stuffed bytes and their lengths of one batch slice; host mode: the
  // images, the streams of one batch slice, the sizes.  plan: the tables and the header of the last (w, h, quality, restart)
  struct JpegSlots {
    enum { kCoef = 0, kBytes, kLens, kIn, kOut, kSizes, kCount };
  };
  struct Jpeg : Lane<JpegSlots> {
    sn::JpgPlan plan;
  } jpg;
  // sn_render / sn_render_jpeg.  host mode: the maps, the left eyes, the canvases at their minimal pitch; sn_render_jpeg: the
  // NV12 canvases of one batch slice, then the encoder's scratch and staging as in JpegSlots, and a plan of its own
  struct RenderSlots {
    enum { kRaw = 0, kLeft, kOut, kCanvas, kCoef, kBytes, kLens, kJpegOut, kSizes, kCount };
  };
  struct Render : Lane<RenderSlots> {
    sn::JpgPlan plan;
  } rnd;
  // sn_obstacles_from_raw.  the beam edges of the last sector (device); host mode: the maps (and their pinned staging), then
  // occ, hits, height_mm, ranges, stats; device mode: hits where the caller wants occ or stats without them
  // sn_obstacles_from_raw_mounts, host mode: the mounts, packed twelve a map
  struct ObstacleSlots {
    enum { kEdges = 0, kRaw, kPinRaw, kOcc, kHits, kHeight, kRanges, kStats, kMounts, kCount };
  };
  struct Obstacles : Lane<ObstacleSlots> {
    Obstacles() { buf[kPinRaw].pinned = true; }
    int beams = 0;                     // the sector whose edges are in buf[kEdges]: 0 = none
    float angle_min = 0.f, angle_increment = 0.f;
  } obs;
  // sn_ground_from_raw.  the hypotheses, their counts and the moments (one allocation each), the per-map state; host mode: the
  // maps (and their pinned staging), the records, the labels; device mode: the records where the caller wants labels alone
  struct GroundSlots {
    enum { kHyp = 0, kCounts, kAcc, kState, kRaw, kPinRaw, kGround, kLabels, kCount };
  };
  struct Ground : Lane<GroundSlots> {
    Ground() { buf[kPinRaw].pinned = true; }
  } gnd;
  // sn_inflate_grid.  the cost table of the last parameter block (device); host mode: occ, cost, grid, dist2, stats
  struct InflateSlots {
    enum { kTable = 0, kOcc, kCost, kGrid, kDist2, kStats, kCount };
  };
  struct Inflate : Lane<InflateSlots> {
    bool cached = false;               // buf[kTable] holds the table of `key`
    sn_inflate_params key{};
  } inf;
  // sn_navfn.  the potential where the caller wants none, the tiles' marks and the work word, the pinned word the host reads it
  // back into; host mode: cost, goals, starts, potential, path, stats
  struct NavSlots {
    enum { kMarks = 0, kPinWork, kCost, kGoals, kStarts, kPot, kPath, kStats, kCount };
  };
  struct Nav : Lane<NavSlots> {
    Nav() { buf[kPinWork].pinned = true; }
  } nav;
  // sn_rollout.  the two tables of (key, key_fp), the samples' words where the caller wants none; host mode: cost, potential,
  // poses, window, samples, best, traj
  struct RolloutSlots {
    enum { kCentres = 0, kOffsets, kCost, kPot, kPoses, kWindow, kSamples, kBest, kTraj, kCount };
  };
  struct Rollout : Lane<RolloutSlots> {
    bool cached = false;               // buf[kCentres] and buf[kOffsets] hold the tables of (key, key_fp[0..2 * key_nf))
    sn_rollout_params key{};
    float key_fp[2 * SN_ROLLOUT_MAX_POINTS] = {};
    int key_nf = 0;
  } roll;
  // The staging of the calls that run on the inference stream (sn_depth_from_raw / sn_mirror_pair_i8 / sn_lr_check /
  // sn_infer_lrc / sn_infer_conf / sn_conf_mask): host-mode copies and the composites' intermediate maps.  Not a lane and no
  // lock: calls on one handle must not overlap.
  struct InferStaging {
    // input tensor, mirrored tensor, left map (masked in place), second map, float map, right map, mask, kept, confidence
    enum { kIn = 0, kMirror, kLeft, kRight, kDisp, kRightOut, kMask, kKept, kConf, kCount };
    GrowBuf buf[kCount];
  } stage;
  std::atomic<int> temporal_live{0};   // sn_temporal objects created on this handle and not yet destroyed: sn_destroy refuses
  std::atomic<int> rectify_live{0};    // ... and sn_rectify objects
  std::atomic<int> costmap_live{0};    // ... and sn_costmap objects
  std::atomic<int> elevation_live{0};  // ... and sn_elevation objects
};

// What the objects with per-stream state on the GPU share (sn_temporal, sn_costmap, sn_elevation)
struct StreamObj {
  sn_handle* h = nullptr;            // nullptr (the two maps only): a host-only object that serves *_pose_q alone
  int streams = 0;
  std::vector<uint8_t> fresh;        // per stream: no frame since create / reset (the kernel then reads no state)
  void open(int n) { streams = n, fresh.assign(n, 1); }
};
// ... and the two rolling maps (the window is p.mw x p.mh of the derived object): per stream the origin of its last frame
struct TorusObj : StreamObj {
  double k256 = 0.0;                 // subs a metre
  std::vector<int> ox, oy;
  void open(int n) { StreamObj::open(n), ox.assign(n, 0), oy.assign(n, 0); }
};

// sn_temporal_*: the one post-processing stage with state: a lane per filter, plus the state planes.  host mode: map (filtered
// in place), guide, float map, mask, counts
struct sn_temporal_slots {
  enum { kRaw = 0, kGuide, kDisp, kMask, kCounts, kCount };
};
struct sn_temporal : Lane<sn_temporal_slots>, StreamObj {
  sn_temporal_params p{};
  long long q = 0;                   // delta_px in units of raw
  void* state = nullptr;             // one allocation: P int32 [streams][H*W], then Hs and Yp uint8 [streams][H*W]
};

// sn_costmap_*: the tail of the chain, with state as sn_temporal: a lane per object, plus the int16 maps and the beam table.
// host mode: occ, ranges, grid, logodds, stats
struct sn_costmap_slots {
  enum { kOcc = 0, kRanges, kGrid, kLog, kStats, kCount };
};
struct sn_costmap : Lane<sn_costmap_slots>, TorusObj {
  sn_costmap_params p{};
  int gw = 0, gh = 0, beams = 0;
  long long gx0 = 0, gy0 = 0, margin = 0, rmin = 0, cmax = 0;
  int16_t* state = nullptr;          // device [streams][mh][mw]
  float* edges = nullptr;            // device [beams + 1]
};

// sn_elevation_*: the 2.5-D map beside the costmap, with state in the same way: a lane per object, plus the two int16 planes.
// kAcc: the accumulators of a call's frames (cnt, fmax, fmin, one plane each); kPlanes: the unrolled hi and lo where the
// caller takes neither (device mode).  host mode: the maps (and their pinned staging), the mounts, trav, hi, lo, rise, stats
struct sn_elevation_slots {
  enum { kAcc = 0, kPlanes, kRaw, kPinRaw, kMounts, kTrav, kHi, kLo, kRise, kStats, kCount };
};
struct sn_elevation : Lane<sn_elevation_slots>, TorusObj {
  sn_elevation() { buf[kPinRaw].pinned = true; }
  sn_elevation_params p{};
  int zmin_mm = 0, zmax_mm = 0;
  int16_t* state = nullptr;          // device: hi [streams][mh][mw], then lo [streams][mh][mw]
};

// sn_rectify_*: the head of the chain: a lane per object, plus the two maps.  host mode: the eyes' source spans (one merged
// span for a side-by-side frame), the rectified frames (also the scratch of a call that wants the tensor alone), the tensors
struct sn_rectify_slots {
  enum { kLeft = 0, kRight, kSbs, kTensor, kCount };
};
struct sn_rectify : Lane<sn_rectify_slots> {
  sn_handle* h = nullptr;
  sn_stereo_calib c{};
  uint32_t valid[2] = {0, 0};
  int32_t* map = nullptr;            // device [2][H][W][2]
};

namespace {

void set_err(const sn_handle* h, const std::string& s) {
  if (h) {
    std::lock_guard<std::mutex> lk(h->err_mu);
    h->err = s;
  }
}
void set_err(std::nullptr_t, const std::string&) {}

template <class T>
hipError_t dalloc(T** p, size_t count) {
  return hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T) + 256);
}

// Device buffers of a parity hook (sn_dbg_*): freed on EVERY return path, error paths included.
struct DevScope {
  std::vector<void*> ptrs;
  void track(const void* p) {
    void* q = const_cast<void*>(p);
    if (q && std::find(ptrs.begin(), ptrs.end(), q) == ptrs.end()) ptrs.push_back(q);
  }
  // count elements of T (dalloc: + 256 bytes), tracked
  template <class T>
  hipError_t alloc(T** p, size_t count) {
    const hipError_t e = dalloc(p, count);
    track(*p);
    return e;
  }
  // the buffers of an uploaded layer; call it whether or not the upload succeeded (a failed one may have allocated some)
  void adopt(const ConvLayer& l) { track(l.wx3); track(l.wpk); track(l.bias); }
  void adopt(const Down0F16& l) { track(l.wfrag); }
  void adopt(const Down01W& l) { track(l.wfrag); track(l.bias); }
  void adopt(const RefLayerF16& l) { track(l.wfrag); track(l.bias); }
  void adopt(const HeadLayer& l) { track(l.w); track(l.pfrag); if (l.wsplit != l.w) track(l.wsplit); }
  ~DevScope() {
    for (void* q : ptrs) (void)hipFree(q);
  }
};

int check_device(sn_handle* h) {
  HIP_TRY(h, hipSetDevice(h->device));
  return SN_OK;
}

}  // namespace
