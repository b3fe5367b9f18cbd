// sn_postproc.hpp — the host side of everything that follows (or wraps) the network: the pieces the entry points share — the
// entry preamble, the k_pre_nv12 launcher, the per-call host staging, the call bracket (Bracket: what opens and closes every
// call, on a lane or on the inference stream), the pair-input staging, the overlap predicates, the guide's geometry — and
// the C ABI of depth, point cloud, mirror, left-right check, confidence, filter, smoother, temporal filter, JPEG encoder, rectifier, render, obstacles, ground plane, costmap, elevation map, inflation, the navigation function and the trajectory rollout.  The kernels are in
// sn_pointcloud.hpp, sn_lrcheck.hpp, sn_confidence.hpp, sn_dispfilter.hpp, sn_smooth.hpp, sn_temporal.hpp, sn_jpeg.hpp, sn_rectify.hpp, sn_render.hpp, sn_obstacles.hpp, sn_ground.hpp, sn_costmap.hpp, sn_elevation.hpp, sn_inflate.hpp, sn_navfn.hpp and sn_rollout.hpp.  Part of the single translation
// unit stereonet_hip.hip.
#pragma once

namespace {

// ---- entry preamble ---------------------------------------------------------------------------------------------------
struct Call {
  hipStream_t st = nullptr;      // the caller's stream, or the default stream of the entry point
  bool host = false;             // SN_MEM_HOST: the call stages its buffers and returns after completion
  bool blocking = false;         // ... as does a device-mode call without a stream of the caller's
};

// What every entry point does after its own argument checks: `mem` is one of the two kinds, the handle's device is current,
// and the call runs on `stream` or else on *own (h->stream; a lane's is created on first use).
int enter(sn_handle* h, const char* where, int mem, void* stream, hipStream_t* own, Call* c) {
  if (mem != SN_MEM_HOST && mem != SN_MEM_DEVICE) {
    set_err(h, std::string(where) + ": bad arguments");
    return SN_ERR_ARG;
  }
  const int rc = check_device(h);
  if (rc) return rc;
  if (!*own) HIP_TRY(h, hipStreamCreateWithFlags(own, hipStreamNonBlocking));
  c->st = stream ? static_cast<hipStream_t>(stream) : *own;
  c->host = mem == SN_MEM_HOST;
  c->blocking = c->host || !stream;
  return SN_OK;
}

// ---- overlap ------------------------------------------------------------------------------------------------------------
struct Span {
  const void* p;
  size_t bytes;
};

// a span of `a` shares a byte with a span of `b` (a null span shares none)
bool overlap(std::initializer_list<Span> a, std::initializer_list<Span> b) {
  for (const Span& x : a)
    for (const Span& y : b) {
      const uintptr_t xl = (uintptr_t)x.p, yl = (uintptr_t)y.p;
      if (xl && yl && xl < yl + y.bytes && yl < xl + x.bytes) return true;
    }
  return false;
}

// The aliasing rule of the calls that mask a map (n maps of HW pixels): of raw, out_raw, disp, mask, counts (`per_map` words a
// map) and the guide's span, only out_raw == raw may share a byte — the one overlap the kernels are written for.
bool masked_map_overlap(size_t n, size_t HW, const int32_t* raw, const int32_t* out_raw, const float* disp, const uint8_t* mask,
                        const uint32_t* counts, int per_map, Span guide = {nullptr, 0}) {
  const Span r{raw, n * HW * 4}, o{out_raw, n * HW * 4}, d{disp, n * HW * 4}, m{mask, n * HW}, k{counts, n * per_map * 4};
  return (out_raw != raw && overlap({r}, {o})) || overlap({r, o}, {d, m, k}) || overlap({d}, {m, k}) || overlap({m}, {k}) ||
         overlap({guide}, {o, d, m, k});
}

// The luma guide of sn_smooth_raw / sn_temporal_push: n NV12 frames in rows of `guide_pitch` bytes, or n int8 model tensors.
// used == false: the call ignores the guide altogether (it may be null, and its span is empty).
struct GuideSpan {
  bool ok;           // the argument test: a known kind, a guide where one is used, an NV12 pitch that is even and >= W
  size_t frame;      // frame k of the guide starts at k * frame
  Span span;         // what the call reads: the luma rows alone, so the last frame ends with the last of them
  int pitch;         // of a luma row
  uint32_t xor_;     // luma = byte ^ xor_: 0 (NV12) or 0x80 (the int8 model input)
  GuideSpan(const sn_handle* h, int n, const void* guide, int kind, int guide_pitch, bool used) {
    const bool nv12 = kind == SN_GUIDE_NV12;
    const size_t HW = (size_t)h->H * h->W;
    ok = !(used && !guide) && (nv12 || kind == SN_GUIDE_TENSOR) && !(nv12 && guide && (guide_pitch < h->W || (guide_pitch & 1)));
    frame = nv12 ? (size_t)guide_pitch * (h->H + (h->H + 1) / 2) : 6 * HW;
    span = used ? Span{guide, (n - 1) * frame + (nv12 ? (size_t)guide_pitch * (h->H - 1) + h->W : HW)} : Span{nullptr, 0};
    pitch = nv12 ? guide_pitch : h->W;
    xor_ = nv12 ? 0u : 0x80u;
  }
};

// The args of the launch that starts at map k0: the per-map pointers of `all` moved on by k0 maps (a luma guide has its own stride)
template <class A>
void at_slice(A& a, const A& all, int k0, size_t HW, int counts_per_map) {
  const size_t off = (size_t)k0 * HW;
  a.raw = all.raw + off;
  a.out_raw = all.out_raw ? all.out_raw + off : nullptr;
  a.disp = all.disp ? all.disp + off : nullptr;
  a.mask = all.mask ? all.mask + off : nullptr;
  a.counts = all.counts ? all.counts + (size_t)k0 * counts_per_map : nullptr;
}

// ---- NV12 input ---------------------------------------------------------------------------------------------------------
// k_pre_nv12 for one pair: the eyes at `left` / `right` in rows of `pitch` bytes -> the int8 tensor `out` (w % 4 == 0 and
// 4-byte aligned pointers are the caller's checks, as is hipGetLastError)
void launch_pre_nv12(hipStream_t st, const uint8_t* left, const uint8_t* right, int pitch, int w, int h_px, int8_t* out) {
  const long total = 6L * h_px * (w >> 2);
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(k_pre_nv12, dim3(blocks), dim3(256), 0, st, left, right, pitch, w, h_px, out);
}

// geometry check of FeedImg (stereonet_node.cpp:682-690) for a side-by-side frame: height == model h, width == 2 * model w
bool sbs_frame_ok(const sn_handle* h, int w2, int h_px) { return w2 / 2 == h->W && h_px == h->H && !(w2 & 7) && !(h_px & 1); }

// FeedImg's split + CvtNV12Data2Tensors for n side-by-side frames -> n int8 tensors at `out` (device).  Host frames go one at
// a time through the workspace's NV12 staging buffer.
int sbs_to_tensors(sn_handle* h, hipStream_t st, int n, const uint8_t* sbs, int w2, int h_px, bool host, int8_t* out) {
  const size_t HW = (size_t)h->H * h->W;
  for (int i = 0; i < n; ++i) {
    const uint8_t* src = sbs + (size_t)i * 3 * HW;
    if (host) {
      HIP_TRY(h, hipMemcpyAsync(h->ws.nv12, src, 3 * HW, hipMemcpyHostToDevice, st));
      src = h->ws.nv12;
    }
    launch_pre_nv12(st, src, src + w2 / 2, w2, w2 / 2, h_px, out + (size_t)i * 6 * HW);
  }
  HIP_TRY(h, hipGetLastError());
  return SN_OK;
}

// ---- host staging of one call ------------------------------------------------------------------------------------------
// Decides the device pointer of every buffer of a call.  Device mode: the caller's.  Host mode: a slot of the feature's
// grow-only buffers, inputs uploaded as they are named, outputs remembered and copied back by download(), all on the call's
// stream and in the order they were named.  A failure sticks in `rc` (SN_ERR_NOMEM for an allocation) and turns everything
// after it into a no-op, so a call names all its buffers and tests `rc` once.
struct Staging {
  sn_handle* h;
  const char* where;      // the entry point, for sn_last_error
  hipStream_t st;
  bool host;
  GrowBuf* slots;         // the feature's buffers, indexed by its enum
  int rc = SN_OK;
  struct Back {
    void* user;
    const void* dev;
    size_t bytes;
  } back[6] = {};
  int n_back = 0;

  int copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, kind, st));
    return SN_OK;
  }
  template <class T>
  T* staged(int which) const { return static_cast<T*>(slots[which].p); }
  // slot `which`, at least `bytes` large, in either mode
  template <class T>
  T* scratch(int which, size_t bytes) {
    if (rc) return nullptr;
    if (slots[which].reserve(bytes) != hipSuccess) {
      set_err(h, std::string(where) + (slots[which].pinned ? ": out of pinned host memory" : ": out of device memory"));
      rc = SN_ERR_NOMEM;
      return nullptr;
    }
    return staged<T>(which);
  }
  template <class T>
  const T* in(int which, const T* user, size_t bytes) {
    if (!host) return user;
    T* d = scratch<T>(which, bytes);
    if (d && (rc = copy(d, user, bytes, hipMemcpyHostToDevice))) return nullptr;
    return d;
  }
  // `in` by way of the pinned slot `pin`: the caller's pages may be pageable, and the call may run beside sn_submit / sn_wait.
  // A host-mode call is blocking, so the one before it is done with the slot.
  template <class T>
  const T* in_pinned(int pin, int which, const T* user, size_t bytes) {
    if (!host) return user;
    void* p = scratch<void>(pin, bytes);
    T* d = scratch<T>(which, bytes);
    if (!d) return nullptr;
    memcpy(p, user, bytes);
    if ((rc = copy(d, p, bytes, hipMemcpyHostToDevice))) return nullptr;
    return d;
  }
  // a nullable output.  needed: the call itself reads it, so it has a device buffer even where the caller wants none
  template <class T>
  T* out(int which, T* user, size_t bytes, bool needed = false) {
    if (user ? !host : !needed) return user;
    return keep(user, scratch<T>(which, bytes), bytes);
  }
  // a nullable buffer the call reads and rewrites in place
  template <class T>
  T* inout(int which, T* user, size_t bytes) {
    if (!host || !user) return user;
    return keep(user, const_cast<T*>(in<T>(which, user, bytes)), bytes);
  }
  // a nullable output that the call writes into `dev`, a buffer it has staged already (host mode: filtered IN PLACE)
  template <class T>
  T* alias(T* user, T* dev, size_t bytes) {
    return host ? keep(user, user ? dev : nullptr, bytes) : user;
  }
  // host mode: download() copies `dev` to `user`
  template <class T>
  T* keep(T* user, T* dev, size_t bytes) {
    if (host && user && dev) back[n_back++] = Back{user, dev, bytes};
    return dev;
  }
  int download() {
    for (int i = 0; i < n_back; ++i)
      if (int e = copy(back[i].user, back[i].dev, back[i].bytes, hipMemcpyDeviceToHost)) return e;
    return SN_OK;
  }
};

// ---- the call bracket ---------------------------------------------------------------------------------------------------
// What every entry point opens after its argument checks and closes once.  Opening, on a lane: lock it, enter(), create its
// event on first use, make the call's stream wait on the event, hand out the Staging `s`.  On the inference stream: enter() and
// the Staging on the handle's InferStaging, no lock and no event (calls on one handle must not overlap).  A failure of the
// opening sticks in s.rc, so an entry point names its buffers and tests s.rc once.  close(): the downloads, the record, the
// sync of a blocking call.  An error exit returns before the record and writes no outputs.
// The order is the same for every lane, and safe for each, because
//   - the wait only enqueues, so nothing the host does after it (growing a buffer, the memcpy into a pinned slot) is held up,
//     and everything the call enqueues after it follows the previous call's last use of the buffers, on whatever stream;
//   - a buffer grows through GrowBuf::reserve, whose hipFree synchronises the device: no earlier call still uses the old one
//     (a first allocation frees nothing, and has no earlier user);
//   - the record follows the downloads, so the next call also waits for them; a call with downloads is a host-mode call, which
//     is blocking and has finished them before it returns.
struct Bracket {
  Call c;
  Staging s;
  std::unique_lock<std::mutex> lk;
  hipEvent_t ev = nullptr;

  Bracket(sn_handle* h, const char* where, int mem, void* stream) : s{h, where, nullptr, false, h->stage.buf} {
    s.rc = enter(h, where, mem, stream, &h->stream, &c);
    s.st = c.st, s.host = c.host;
  }
  template <class L>
  Bracket(sn_handle* h, const char* where, int mem, void* stream, L& lane) : s{h, where, nullptr, false, lane.buf}, lk(lane.mu) {
    s.rc = open(mem, stream, lane.stream, lane.ev);
    ev = lane.ev;
  }
  int open(int mem, void* stream, hipStream_t& own, hipEvent_t& lane_ev) {
    if (int rc = enter(s.h, s.where, mem, stream, &own, &c)) return rc;
    s.st = c.st, s.host = c.host;
    if (!lane_ev) HIP_TRY(s.h, hipEventCreateWithFlags(&lane_ev, hipEventDisableTiming));
    HIP_TRY(s.h, hipStreamWaitEvent(c.st, lane_ev, 0));
    return SN_OK;
  }
  int close() {
    if (int e = s.download()) return e;
    if (ev) HIP_TRY(s.h, hipEventRecord(ev, c.st));
    if (c.blocking) HIP_TRY(s.h, hipStreamSynchronize(c.st));
    return SN_OK;
  }
};

// The `in` of sn_infer_lrc / sn_infer_conf — n int8 model tensors or n side-by-side NV12 frames, host or device — checked ...
int pair_input_check(sn_handle* h, const char* where, const void* in, int in_kind, int w2, int h_px, int mem) {
  if (in_kind != SN_LRC_IN_TENSOR && in_kind != SN_LRC_IN_SBS_NV12) {
    set_err(h, std::string(where) + ": bad arguments");
    return SN_ERR_ARG;
  }
  if (in_kind == SN_LRC_IN_SBS_NV12 && (!sbs_frame_ok(h, w2, h_px) || (mem == SN_MEM_DEVICE && ((uintptr_t)in & 3)))) {
    set_err(h, std::string(where) + ": image size does not match the model input");
    return SN_ERR_ARG;
  }
  return SN_OK;
}

// ... and brought to the device as tensors (s.rc on failure)
const int8_t* pair_input(Staging& s, int n, const void* in, int in_kind, int w2, int h_px) {
  using S = sn_handle::InferStaging;
  const size_t bytes = (size_t)n * 6 * s.h->H * s.h->W;
  if (in_kind != SN_LRC_IN_SBS_NV12) return s.in(S::kIn, static_cast<const int8_t*>(in), bytes);
  int8_t* ten = s.scratch<int8_t>(S::kIn, bytes);
  if (ten && (s.rc = sbs_to_tensors(s.h, s.st, n, static_cast<const uint8_t*>(in), w2, h_px, s.host, ten))) return nullptr;
  return ten;
}

// ---- kernel launches (device pointers) ---------------------------------------------------------------------------------
// the camera test of sn_pointcloud_from_raw and sn_obstacles_from_raw
bool camera_ok(const sn_camera* cam) {
  return cam && cam->fx > 0.f && std::isfinite(cam->fx) && cam->fy > 0.f && std::isfinite(cam->fy) && cam->baseline_mm > 0.f &&
         (cam->step == 1 || cam->step == 2 || cam->step == 4);
}

// nullptr, or why sn_obstacles_from_raw refuses the parameters (the sector of a scan is ob_beam_edges' test)
const char* obstacle_params_check(const sn_obstacle_params* p) {
  if (!p) return "a NULL pointer";
  for (float v : p->base_from_cam)
    if (!std::isfinite(v)) return "base_from_cam must be finite";
  for (float v : {p->x_min_m, p->y_min_m, p->cell_m, p->z_floor_m, p->z_lo_m, p->z_hi_m, p->angle_min_rad, p->angle_increment_rad,
                  p->range_min_m, p->range_max_m})
    if (!std::isfinite(v)) return "every parameter must be finite";
  if (!(p->cell_m > 0.f)) return "cell_m must be positive";
  if (p->gw < 0 || p->gh < 0 || p->gw > kObMaxCells || p->gh > kObMaxCells || (p->gw == 0) != (p->gh == 0))
    return "gw and gh must be 1..4096, or both 0";
  if (p->beams < 0 || p->beams > kObMaxBeams) return "beams must be 0..4096";
  if (p->z_floor_m > p->z_lo_m || p->z_lo_m > p->z_hi_m) return "z_floor_m <= z_lo_m <= z_hi_m is required";
  if (p->min_obstacle_hits < 0 || p->min_ground_hits < 0) return "the hit thresholds must not be negative";
  if (p->range_min_m < 0.f || p->range_max_m < p->range_min_m) return "0 <= range_min_m <= range_max_m is required";
  return nullptr;
}

bool lrc_params_ok(const sn_lrc_params* p) {
  return p && std::isfinite(p->tau_px) && std::isfinite(p->tau_rel) && p->tau_px >= 0.f && p->tau_rel >= 0.f;
}

bool conf_params_ok(const sn_conf_params* p) {
  return p && std::isfinite(p->min_conf) && p->min_conf >= 0.f && p->min_conf <= 1.f;
}

int mirror_launch(sn_handle* h, hipStream_t st, int n, const int8_t* in, int8_t* out) {
  MirrorArgs a{in, out, n, h->H, h->W};
  const bool vec = (h->W & 15) == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
  const size_t items = (size_t)n * 6 * h->H * (vec ? h->W >> 4 : h->W);
  const unsigned grid = (unsigned)std::min<size_t>((items + 255) / 256, 8192);
  if (vec) hipLaunchKernelGGL(k_mirror_pair<true>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_mirror_pair<false>, dim3(grid), dim3(256), 0, st, a);
  HIP_TRY(h, hipGetLastError());
  return SN_OK;
}

// right_out (nullable) receives the right map in right-image coordinates
int lrc_launch(sn_handle* h, hipStream_t st, int n, const int32_t* left, const int32_t* right, const sn_lrc_params* p,
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

// low: conf_in is a low-resolution plane [n][hl][wl] (upsampled, out_conf nullable); else a full-resolution map.
// p == nullptr: no masking (out_conf only)
int conf_launch(sn_handle* h, hipStream_t st, int n, bool low, const float* conf_in, const int32_t* raw, const sn_conf_params* p,
                float* out_conf, int32_t* out_raw, float* disp, uint8_t* mask, uint32_t* kept) {
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

// The three launches for m frames on device pointers: dct == nullptr except for the debug hook
int jpeg_launch(sn_handle* h, hipStream_t st, const JpgPlan& plan, int m, const uint8_t* nv12, int pitch, size_t frame,
                int rows_per_slice, int16_t* coef, uint8_t* bytes, uint32_t* lens, uint8_t* out, size_t out_stride, uint32_t* sizes,
                float* dct = nullptr) {
  const int w = plan.w, hp = plan.h, mw = (w + 15) / 16, rows = jpg_mcu_rows(hp), blocks = mw * rows * 6;
  JpgDctArgs d{nv12, coef, dct, frame, pitch, w, hp, mw, blocks, {}, {}};
  memcpy(d.rl, plan.rl, sizeof d.rl);
  memcpy(d.rc, plan.rc, sizeof d.rc);
  hipLaunchKernelGGL(k_jpeg_dct, dim3((blocks + 255) / 256, m), dim3(256), 0, st, d);
  if (out) {
    const int per = plan.restart ? plan.restart * 6 : blocks, nslices = plan.restart ? (rows + rows_per_slice - 1) / rows_per_slice : 1;
    const size_t cap = (size_t)per * (2 * kJpgBlockBytes) + 16;
    JpgEntArgs e{coef, bytes, lens, cap, blocks, per, nslices, {}};
    memcpy(e.huff, plan.huff, sizeof e.huff);
    hipLaunchKernelGGL(k_jpeg_entropy, dim3(nslices, m), dim3(kJpgT), 0, st, e);
    JpgAsmArgs a{bytes, lens, out, sizes, out_stride, cap, nslices, plan.hdr_len, {}};
    memcpy(a.hdr, plan.hdr, sizeof a.hdr);
    hipLaunchKernelGGL(k_jpeg_assemble, dim3(nslices, m), dim3(256), 0, st, a);
  }
  HIP_TRY(h, hipGetLastError());
  return SN_OK;
}

// The encoder's walk over the n frames of a call on an open bracket, shared by sn_jpeg_encode_nv12 and sn_render_jpeg: the
// scratch of one batch slice in the lane's slots `id`, then per slice `source(k0, m, &src)` (the slice's first frame, after
// enqueuing whatever makes it), the three launches and, in host mode, the copy of every stream by its size.
struct JpgSlotIds {
  int coef, bytes, lens, out, sizes;
};

template <class Source>
int jpeg_walk(sn_handle* h, Staging& s, hipStream_t st, JpgPlan& plan, const JpgSlotIds& id, int n, int w, int h_px, int pitch,
              size_t frame, const sn_jpeg_params* p, int restart, uint8_t* out, size_t out_stride, uint32_t* sizes, Source source) {
  jpg_make_plan(w, h_px, p->quality, restart, &plan);
  const size_t bound = jpg_bound(w, h_px);
  const int mw = (w + 15) / 16, rows = jpg_mcu_rows(h_px), blocks = mw * rows * 6;
  const int per = restart ? restart * 6 : blocks, nslices = restart ? (rows + p->rows_per_slice - 1) / p->rows_per_slice : 1;
  const int slice = std::min(h->max_batch, kJpgSlice);
  int16_t* coef = s.scratch<int16_t>(id.coef, (size_t)slice * blocks * 128);
  uint8_t* bytes = s.scratch<uint8_t>(id.bytes, (size_t)slice * nslices * ((size_t)per * (2 * kJpgBlockBytes) + 16));
  uint32_t* lens = s.scratch<uint32_t>(id.lens, (size_t)slice * nslices * 4);
  // host mode: the streams of one batch slice are staged at a stride no stream needs more than, and copied back by their sizes
  const size_t dstride = s.host ? std::min(out_stride, bound) : out_stride;
  uint8_t* dout = s.host ? s.scratch<uint8_t>(id.out, (size_t)slice * dstride + 16) : out;
  uint32_t* dsizes = s.host ? s.scratch<uint32_t>(id.sizes, (size_t)n * 4) : sizes;
  if (s.rc) return s.rc;
  for (int k0 = 0; k0 < n; k0 += slice) {      // the scratch holds `slice` frames: walk the batch on the stream
    const int m = std::min(slice, n - k0);
    const uint8_t* src = nullptr;
    if (int rc = source(k0, m, &src)) return rc;
    if (int rc = jpeg_launch(h, st, plan, m, src, pitch, frame, p->rows_per_slice, coef, bytes, lens,
                             s.host ? dout : dout + (size_t)k0 * out_stride, dstride, dsizes + k0))
      return rc;
    if (s.host) {
      if (int e = s.copy(sizes + k0, dsizes + k0, (size_t)m * 4, hipMemcpyDeviceToHost)) return e;
      HIP_TRY(h, hipStreamSynchronize(st));
      for (int k = 0; k < m; ++k)
        if (sizes[k0 + k])
          if (int e = s.copy(out + (size_t)(k0 + k) * out_stride, dout + (size_t)k * dstride, sizes[k0 + k], hipMemcpyDeviceToHost))
            return e;
      HIP_TRY(h, hipStreamSynchronize(st));      // the next slice rewrites the staged streams
    }
  }
  return SN_OK;
}

// sn_render / sn_render_jpeg: the checked arguments of a call
struct RenderCall {
  sn_render_params p;      // the zero fields replaced by the reference's values
  bool nv12, stack;
  int Hc, rows, row_bytes;      // canvas rows (NV12: luma and chroma), the bytes the call writes in each
  size_t raw_bytes, left_frame, left_span;
};

// nullptr, or why the arguments are refused
const char* render_check(const sn_handle* h, int n, const int32_t* raw, const uint8_t* left, int left_pitch, const sn_render_params* p,
                         int format, RenderCall* c) {
  if (!raw || !p) return "a NULL pointer";
  if (n <= 0 || n > h->max_batch) return "n outside 1..max_batch";
  if (p->layout != SN_RENDER_STACK && p->layout != SN_RENDER_DEPTH) return "unknown layout";
  if (format != SN_RENDER_RGB8 && format != SN_RENDER_NV12) return "unknown format";
  if (p->colormap != SN_CMAP_JET && p->colormap != SN_CMAP_GREY) return "unknown colour map";
  for (double v : {p->scale, p->focal_px, p->baseline_mm})
    if (!std::isfinite(v) || v < 0) return "scale, focal_px and baseline_mm must be finite and not negative";
  if (!std::isfinite(p->alpha)) return "alpha must be finite";
  c->p = *p;
  if (c->p.scale == 0) c->p.scale = 0.00000260443857769133;
  if (c->p.focal_px == 0) c->p.focal_px = 527.1931762695312;
  if (c->p.baseline_mm == 0) c->p.baseline_mm = 119.89382172;
  if (c->p.alpha == 0) c->p.alpha = 9.0;
  c->nv12 = format == SN_RENDER_NV12;
  c->stack = p->layout == SN_RENDER_STACK;
  if (c->stack && !left) return "SN_RENDER_STACK needs left_nv12";
  if (c->stack && (left_pitch < h->W || (left_pitch & 1))) return "left_pitch must be even and >= W";
  if (c->nv12 && ((h->W | h->H) & 1)) return "SN_RENDER_NV12 needs an even width and height";
  c->Hc = c->stack ? 2 * h->H : h->H;
  c->rows = c->nv12 ? c->Hc + c->Hc / 2 : c->Hc;
  c->row_bytes = c->nv12 ? h->W : 3 * h->W;
  c->raw_bytes = (size_t)n * h->H * h->W * 4;
  const int left_rows = h->H + (h->H + 1) / 2;      // an odd height has ceil(H/2) chroma rows
  c->left_frame = c->stack ? (size_t)left_pitch * left_rows : 0;
  c->left_span = c->stack ? (n - 1) * c->left_frame + (size_t)(left_rows - 1) * left_pitch + ((h->W + 1) & ~1) : 0;
  return nullptr;
}

// one launch: n canvases at device pointers
int render_launch(sn_handle* h, hipStream_t st, int n, const RenderCall& c, const int32_t* raw, const uint8_t* left, int left_pitch,
                  uint8_t* out, int out_pitch, size_t out_frame) {
  RenderArgs a{};
  a.raw = raw, a.left = c.stack ? left : nullptr, a.out = out;
  a.left_frame = c.left_frame, a.out_frame = out_frame;
  a.scale = c.p.scale, a.fB = c.p.focal_px * c.p.baseline_mm, a.alpha = c.p.alpha;
  a.W = h->W, a.H = h->H, a.left_pitch = left_pitch, a.out_pitch = out_pitch;
  a.stack = c.stack, a.invalid_black = c.p.invalid_black != 0;
  a.vec_raw = (h->W & 3) == 0 && ((uintptr_t)raw & 15) == 0;
  a.word_left = c.stack && (((uintptr_t)left | (size_t)left_pitch | c.left_frame) & 3) == 0;
  a.word_out = (((uintptr_t)out | (size_t)out_pitch | out_frame) & 3) == 0;
  uint8_t tab[kRenderEntries * 3];
  render_tables(&c.p, c.nv12 ? nullptr : tab, c.nv12 ? tab : nullptr);
  for (int i = 0; i < kRenderEntries; ++i) a.tab[i] = tab[3 * i] | (uint32_t)tab[3 * i + 1] << 8 | (uint32_t)tab[3 * i + 2] << 16;
  const int items = ((h->W + 3) / 4) * ((h->H + 1) / 2);
  const dim3 grid((items + 255) / 256, n);
  if (c.nv12) hipLaunchKernelGGL(k_render<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_render<false>, grid, dim3(256), 0, st, a);
  HIP_TRY(h, hipGetLastError());
  return SN_OK;
}


// ---- the objects with per-stream state (sn_engine.hpp's StreamObj and TorusObj): what sn_temporal_*, sn_costmap_* and
// sn_elevation_* share.  The grouping of a push, its commit and the pose rule are in csrc/sn_stream_groups.hpp ------------------
bool streams_ok(const sn_handle* h, int streams) { return streams >= 1 && (!h || streams <= h->max_batch); }

// The tail of a create: the per-stream flags, and on a handle the device check, the allocations (all or none) and the live count
template <class T>
int stream_open(T* o, sn_handle* h, int streams, const char* who, std::atomic<int> sn_handle::*live,
                std::initializer_list<std::pair<void**, size_t>> dev) {
  o->h = h;
  o->open(streams);
  if (!h) return SN_OK;
  if (const int rc = check_device(h)) return rc;
  for (const auto& d : dev)
    if (hipMalloc(d.first, d.second) != hipSuccess) {
      (void)hipGetLastError();
      for (const auto& u : dev) (void)hipFree(*u.first), *u.first = nullptr;
      set_err(h, std::string(who) + ": out of device memory");
      return SN_ERR_NOMEM;
    }
  ++(h->*live);
  return SN_OK;
}

template <class T>
int stream_reset(T* o, int stream, const char* who) {
  if (!o) return SN_ERR_ARG;
  if (stream < -1 || stream >= o->streams) {
    set_err(o->h, std::string(who) + ": bad arguments");
    return SN_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(o->mu);
  if (stream < 0) std::fill(o->fresh.begin(), o->fresh.end(), (uint8_t)1);
  else o->fresh[stream] = 1;
  return SN_OK;
}

// dev: the members that hold the object's device allocations
template <class T, class... M>
void stream_destroy(T* o, std::atomic<int> sn_handle::*live, M T::*... dev) {
  if (!o) return;
  if (o->h) {      // not a host-only object
    (void)hipSetDevice(o->h->device);
    o->destroy();
    ((void)hipFree(o->*dev), ...);
    --(o->h->*live);
  }
  delete o;
}

// the contract's q of one pose on a rolling map's window; false where sn_costmap_pose_q / sn_elevation_pose_q refuse it
template <class T>
bool torus_pose_q(const T* o, const double* pose, int32_t* q) { return sn::torus_pose_q(o->k256, o->p.mw, o->p.mh, pose, q); }
}  // namespace

extern "C" {

// ---- depth: Parse's dequantisation (k_depth_from_raw), on the inference stream; host mode stages in InferStaging's slots of
// the left map (raw), the float map (depth) and the confidence (disp_px), so an allocation failure is SN_ERR_NOMEM ------------
int sn_depth_from_raw(sn_handle* h, int n, const int32_t* raw, float focal_px, float baseline_mm, float* depth_m, float* disp_px,
                      int mem, void* stream) {
  if (!h || !raw || !depth_m || n <= 0 || n > h->max_batch) return SN_ERR_ARG;
  Bracket b(h, "sn_depth_from_raw", mem, stream);
  Staging& s = b.s;
  using S = sn_handle::InferStaging;
  const size_t cnt = (size_t)n * h->H * h->W;
  const float fB = focal_px * baseline_mm;      // float product, as in the reference expression
  const int32_t* draw = s.in(S::kLeft, raw, cnt * 4);
  float* ddepth = s.out(S::kDisp, depth_m, cnt * 4);
  float* ddisp = s.out(S::kConf, disp_px, cnt * 4);
  if (s.rc) return s.rc;
  unsigned grid = (unsigned)((cnt + 255) / 256);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(k_depth_from_raw, dim3(grid), dim3(256), 0, b.c.st, draw, cnt, kOutScale, fB, ddepth, ddisp);
  HIP_TRY(h, hipGetLastError());
  return b.close();
}

// ---- point cloud (csrc/sn_pointcloud.hpp): a lane of the handle's; host mode stages through pinned memory --------------------
// An allocation failure is SN_ERR_NOMEM, as in every other stage.
int sn_pointcloud_from_raw(sn_handle* h, int n, const int32_t* raw, const uint8_t* nv12, int nv12_pitch, const sn_camera* cam,
                           int layout, float* points, uint32_t* counts, int mem, void* stream) {
  if (!h || !raw || !cam || !points || n <= 0 || n > h->max_batch || ((uintptr_t)points & 15) ||
      (layout != SN_PC_ORGANISED && layout != SN_PC_COMPACT) || (layout == SN_PC_COMPACT && !counts))
    return SN_ERR_ARG;
  if (!camera_ok(cam)) return SN_ERR_ARG;
  if (nv12 && (nv12_pitch < h->W || (nv12_pitch & 1))) return SN_ERR_ARG;
  using P = sn_handle::PointCloud;
  Bracket b(h, "sn_pointcloud_from_raw", mem, stream, h->pc);
  Staging& s = b.s;
  hipStream_t st = b.c.st;
  const int W = h->W, H = h->H, step = cam->step;
  const int Wo = (W + step - 1) / step, Ho = (H + step - 1) / step;
  const int tiles = (Ho * Wo + kPcTile - 1) / kPcTile;
  const size_t raw_bytes = (size_t)n * H * W * 4, pts_bytes = (size_t)n * Ho * Wo * 16;
  const size_t frame = (size_t)nv12_pitch * (H + (H + 1) / 2);    // an odd height has ceil(H/2) chroma rows
  const bool compact = layout == SN_PC_COMPACT;
  uint32_t* scratch = compact ? s.scratch<uint32_t>(P::kScratch, (size_t)n * tiles * 4) : s.staged<uint32_t>(P::kScratch);
  const int32_t* draw = s.in_pinned(P::kPinRaw, P::kRaw, raw, raw_bytes);
  const uint8_t* dnv12 = nv12 ? s.in_pinned(P::kPinNv12, P::kNv12, nv12, n * frame) : nullptr;
  // compact, host mode: the counts say how much of every map to copy, so both are copied below and not by download()
  const bool by_hand = compact && s.host;
  float4* dpts = by_hand ? s.scratch<float4>(P::kPoints, pts_bytes) : s.out(P::kPoints, reinterpret_cast<float4*>(points), pts_bytes);
  uint32_t* dcounts = by_hand ? s.scratch<uint32_t>(P::kCounts, (size_t)n * 4) : s.out(P::kCounts, counts, (size_t)n * 4);
  if (s.rc) return s.rc;
  PcArgs a{draw, dnv12, dpts, dcounts, scratch, frame, W, H, Wo, Ho, step, nv12_pitch, tiles, kOutScale,
           cam->fx * cam->baseline_mm, cam->fx, cam->fy, cam->cx, cam->cy, cam->z_min_m, cam->z_max_m, 0};
  a.vec = step == 1 && (W & 3) == 0 && ((uintptr_t)a.raw & 15) == 0;
  if (!compact) {
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
  if (by_hand) {
    if (int e = s.copy(counts, dcounts, (size_t)n * 4, hipMemcpyDeviceToHost)) return e;
    HIP_TRY(h, hipStreamSynchronize(st));
    for (int k = 0; k < n; ++k) {
      const int e = counts[k] ? s.copy(points + (size_t)k * Ho * Wo * 4, dpts + (size_t)k * Ho * Wo, (size_t)counts[k] * 16,
                                       hipMemcpyDeviceToHost) : SN_OK;
      if (e) return e;
    }
  }
  return b.close();
}

// ---- obstacle grid and laser scan (csrc/sn_obstacles.hpp): a lane of the handle's; host mode stages the maps through pinned
// memory as the point cloud does ------------------------------------------------------------------------------------------------
int sn_obstacle_beam_edges(const sn_obstacle_params* p, float* edges) {
  return p && edges && ob_beam_edges(p->beams, p->angle_min_rad, p->angle_increment_rad, edges) ? SN_OK : SN_ERR_ARG;
}

namespace {
// both entry points.  mounts: nullptr (p->base_from_cam is the mount of every map), or a mount per map
int obstacles_call(sn_handle* h, const char* where, int n, const int32_t* raw, const sn_camera* cam, const sn_obstacle_params* p_in,
                   const float* mounts, int mount_stride, int8_t* occ, uint32_t* hits, int32_t* height_mm, float* ranges, uint32_t* stats,
                   int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  auto refuse = [&](const char* why) {
    set_err(h, std::string(where) + ": " + why);
    return SN_ERR_ARG;
  };
  if (!raw || !p_in) return refuse("a NULL pointer");
  sn_obstacle_params with_mounts;
  if (mounts) {      // p->base_from_cam is ignored
    with_mounts = *p_in;
    for (float& v : with_mounts.base_from_cam) v = 0.f;
  }
  const sn_obstacle_params* p = mounts ? &with_mounts : p_in;
  if (n <= 0 || n > h->max_batch) return refuse("n outside 1..max_batch");
  if (!camera_ok(cam)) return refuse("a camera sn_pointcloud_from_raw refuses");
  if (const char* why = obstacle_params_check(p)) return refuse(why);
  if (!occ && !hits && !height_mm && !ranges) return refuse("one of occ, hits, height_mm and ranges is needed");
  if ((occ || hits || height_mm || stats) && !p->gw) return refuse("occ, hits, height_mm and stats need a grid (gw, gh > 0)");
  if (ranges && !p->beams) return refuse("ranges needs beams > 0");
  std::vector<float> edges;
  if (ranges) {
    edges.resize(p->beams + 1);
    if (!ob_beam_edges(p->beams, p->angle_min_rad, p->angle_increment_rad, edges.data()))
      return refuse("the sector must lie inside (-pi/2, pi/2) with strictly increasing edges");
  }
  const int W = h->W, H = h->H, step = cam->step;
  const int Wo = (W + step - 1) / step, Ho = (H + step - 1) / step;
  const size_t cells = (size_t)p->gw * p->gh, raw_bytes = (size_t)n * H * W * 4;
  const size_t occ_bytes = n * cells, hits_bytes = n * cells * 8, height_bytes = n * cells * 4, ranges_bytes = (size_t)n * p->beams * 4,
               stats_bytes = (size_t)n * 16;
  const size_t mounts_bytes = mounts ? ((size_t)(n - 1) * mount_stride + 12) * 4 : 0;
  {
    const Span in{raw, raw_bytes};
    const Span out[5] = {{occ, occ_bytes}, {hits, hits_bytes}, {height_mm, height_bytes}, {ranges, ranges_bytes}, {stats, stats_bytes}};
    for (int i = 0; i < 5; ++i) {
      if (overlap({in, Span{mounts, mounts_bytes}}, {out[i]})) return refuse("overlapping buffers");
      for (int j = i + 1; j < 5; ++j)
        if (overlap({out[i]}, {out[j]})) return refuse("overlapping buffers");
    }
  }
  using O = sn_handle::Obstacles;
  O& lane = h->obs;
  Bracket b(h, where, mem, stream, lane);
  Staging& s = b.s;
  hipStream_t st = b.c.st;
  const bool grid = occ || hits || height_mm || stats;
  const int32_t* draw = s.in_pinned(O::kPinRaw, O::kRaw, raw, raw_bytes);
  int8_t* docc = s.out(O::kOcc, occ, occ_bytes);
  uint32_t* dhits = s.out(O::kHits, hits, hits_bytes, grid);      // every grid output comes from the counts
  int32_t* dheight = s.out(O::kHeight, height_mm, height_bytes);
  uint32_t* dranges = s.out(O::kRanges, reinterpret_cast<uint32_t*>(ranges), ranges_bytes);
  uint32_t* dstats = s.out(O::kStats, stats, stats_bytes);
  std::vector<float> packed;      // host mode: the mounts, twelve a map (the call is blocking, so it outlives the copy)
  const float* dmounts = mounts;
  if (mounts && s.host) {
    packed.resize((size_t)n * 12);
    for (int k = 0; k < n; ++k) memcpy(&packed[(size_t)k * 12], mounts + (size_t)k * mount_stride, 48);
    dmounts = s.in(O::kMounts, packed.data(), packed.size() * 4);
  }
  const bool same_sector = ranges && lane.beams == p->beams && lane.angle_min == p->angle_min_rad &&
                           lane.angle_increment == p->angle_increment_rad;
  float* dedges = ranges ? s.scratch<float>(O::kEdges, (size_t)(kObMaxBeams + 1) * 4) : nullptr;
  if (s.rc) return s.rc;
  if (ranges && !same_sector) {      // a new sector is rare: its table is uploaded behind the lane's earlier calls and waited for
    lane.beams = 0;
    HIP_TRY(h, hipMemcpyAsync(dedges, edges.data(), edges.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    lane.beams = p->beams, lane.angle_min = p->angle_min_rad, lane.angle_increment = p->angle_increment_rad;
  }
  ObArgs a{};
  a.pc.raw = draw;
  a.pc.W = W, a.pc.H = H, a.pc.Wo = Wo, a.pc.Ho = Ho, a.pc.step = step;
  a.pc.scale = kOutScale, a.pc.fB = cam->fx * cam->baseline_mm, a.pc.fx = cam->fx, a.pc.fy = cam->fy, a.pc.cx = cam->cx, a.pc.cy = cam->cy;
  a.pc.zmin = cam->z_min_m, a.pc.zmax = cam->z_max_m;
  a.edges = dedges, a.hits = dhits, a.height = dheight, a.ranges = dranges;
  bool level = true;
  for (float v : p->base_from_cam) level = level && v == 0.f;
  const float level_mount[12] = {0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0};
  memcpy(a.m, level ? level_mount : p->base_from_cam, sizeof a.m);
  a.mounts = dmounts, a.mount_stride = mounts && s.host ? 12 : mount_stride;
  a.x_min = p->x_min_m, a.y_min = p->y_min_m, a.cell = p->cell_m, a.z_floor = p->z_floor_m, a.z_lo = p->z_lo_m, a.z_hi = p->z_hi_m;
  a.r_min = p->range_min_m, a.r_max = p->range_max_m;
  a.gw = p->gw, a.gh = p->gh, a.beams = ranges ? p->beams : 0;
  // a workgroup is 256 columns of a chunk of rows: about 2048 workgroups a call, and runs of at least 16 rows
  const int cblocks = (Wo + 255) / 256;
  a.chunks = std::max(1, std::min((2048 + cblocks * n - 1) / (cblocks * n), (Ho + 15) / 16));
  a.rows = (Ho + a.chunks - 1) / a.chunks;
  a.chunks = (Ho + a.rows - 1) / a.rows;
  {
    const ObFillArgs f{dhits, dstats, dheight, dranges, dhits ? n * cells * 2 : 0, dstats ? (size_t)n * 4 : 0, dheight ? n * cells : 0,
                       dranges ? (size_t)n * p->beams : 0};
    const size_t words = f.n_hits + f.n_stats + f.n_height + f.n_ranges;
    hipLaunchKernelGGL(k_ob_fill, dim3((unsigned)std::min<size_t>((words + 255) / 256, 2048)), dim3(256), 0, st, f);
  }
  const dim3 acc_grid(cblocks * a.chunks, n);
  const size_t lds = dranges ? ((h->obstacle_rle ? 2 : 1) * a.beams + 1) * 4 : 0;
  if (h->obstacle_rle && mounts) hipLaunchKernelGGL((k_ob_accumulate<true, true>), acc_grid, dim3(256), lds, st, a);
  else if (h->obstacle_rle) hipLaunchKernelGGL((k_ob_accumulate<true, false>), acc_grid, dim3(256), lds, st, a);
  else if (mounts) hipLaunchKernelGGL((k_ob_accumulate<false, true>), acc_grid, dim3(256), lds, st, a);
  else hipLaunchKernelGGL((k_ob_accumulate<false, false>), acc_grid, dim3(256), lds, st, a);
  if (docc || dstats) {
    ObClassArgs c{dhits, docc, dstats, (int)cells, p->min_obstacle_hits, p->min_ground_hits};
    const int per_map = (int)std::max<size_t>(1, std::min<size_t>((cells + 255) / 256, 1024 / n));
    hipLaunchKernelGGL(k_ob_classify, dim3(per_map, n), dim3(256), 0, st, c);
  }
  HIP_TRY(h, hipGetLastError());
  return b.close();
}
}  // namespace

int sn_obstacles_from_raw(sn_handle* h, int n, const int32_t* raw, const sn_camera* cam, const sn_obstacle_params* p, int8_t* occ,
                          uint32_t* hits, int32_t* height_mm, float* ranges, uint32_t* stats, int mem, void* stream) {
  return obstacles_call(h, "sn_obstacles_from_raw", n, raw, cam, p, nullptr, 0, occ, hits, height_mm, ranges, stats, mem, stream);
}

int sn_obstacles_from_raw_mounts(sn_handle* h, int n, const int32_t* raw, const sn_camera* cam, const sn_obstacle_params* p,
                                 const float* mounts, int mount_stride, int8_t* occ, uint32_t* hits, int32_t* height_mm, float* ranges,
                                 uint32_t* stats, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  if (!mounts || ((uintptr_t)mounts & 3) || mount_stride < 12) {
    set_err(h, "sn_obstacles_from_raw_mounts: mounts must be a 4-byte aligned pointer with mount_stride >= 12");
    return SN_ERR_ARG;
  }
  return obstacles_call(h, "sn_obstacles_from_raw_mounts", n, raw, cam, p, mounts, mount_stride, occ, hits, height_mm, ranges, stats,
                        mem, stream);
}

// ---- ground plane (csrc/sn_ground.hpp): a lane of the handle's, staged as the obstacle stage ---------------------------------
namespace {
// nullptr, or why sn_ground_from_raw refuses the parameters (the region apart: gr_roi says)
const char* ground_params_check(const sn_camera* cam, const sn_ground_params* p, int64_t* tol) {
  if (!p) return "a NULL pointer";
  if (!camera_ok(cam) || !std::isfinite(cam->cx) || !std::isfinite(cam->cy)) return "a camera sn_pointcloud_from_raw refuses, or cx, cy not finite";
  for (float v : p->base_from_cam)
    if (!std::isfinite(v)) return "base_from_cam must be finite";
  for (float v : {p->tol_px, p->max_tilt_rad, p->height_min_m, p->height_max_m})
    if (!std::isfinite(v)) return "every parameter must be finite";
  if (p->hypotheses < 1 || p->hypotheses > kGrMaxHyp) return "hypotheses must be 1..1024";
  if (p->refits < 0 || p->refits > kGrMaxRefits) return "refits must be 0..4";
  if (p->min_area < 0 || p->min_inliers < 0) return "min_area and min_inliers must not be negative";
  if (p->tol_px < 0.f) return "tol_px must not be negative";
  const float q = floorf(p->tol_px / gr_scale(kOutScale));      // sn_temporal's rule
  if (!(q <= (float)kGrMaxRaw)) return "tol_px is too large (tol_raw <= 2^24)";
  *tol = (int64_t)q;
  if (p->max_tilt_rad < 0.f || p->max_tilt_rad > 1.5f) return "max_tilt_rad must lie in [0, 1.5]";
  if (!(p->height_min_m > 0.f) || p->height_max_m < p->height_min_m) return "0 < height_min_m <= height_max_m is required";
  return nullptr;
}
}  // namespace

int sn_ground_gate(const sn_camera* cam, const sn_ground_params* p, int W, int H, int64_t gate[6]) {
  int64_t tol;
  GrRoi roi;
  if (!gate || W < 1 || H < 1 || W > 8192 || H > 8192 || ground_params_check(cam, p, &tol) || gr_roi(p, W, H, cam->step, &roi))
    return SN_ERR_ARG;
  gr_gate(cam, p, roi, kOutScale, gate);
  return SN_OK;
}

int sn_ground_from_raw(sn_handle* h, int n, const int32_t* raw, const sn_camera* cam, const sn_ground_params* p, sn_ground* ground,
                       uint8_t* labels, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  auto refuse = [&](const char* why) {
    set_err(h, std::string("sn_ground_from_raw: ") + why);
    return SN_ERR_ARG;
  };
  if (!raw || !cam) return refuse("a NULL pointer");
  if (n <= 0 || n > h->max_batch) return refuse("n outside 1..max_batch");
  GrArgs a{};
  if (const char* why = ground_params_check(cam, p, &a.tol)) return refuse(why);
  const int W = h->W, H = h->H;
  if (W > 8192 || H > 8192) return refuse("maps beyond 8192 x 8192");
  if (const char* why = gr_roi(p, W, H, cam->step, &a.roi)) return refuse(why);
  if (!ground && !labels) return refuse("one of ground and labels is needed");
  if ((uintptr_t)ground & 7) return refuse("ground must be 8-byte aligned");
  const size_t HW = (size_t)H * W, raw_bytes = n * HW * 4, ground_bytes = (size_t)n * sizeof(sn_ground), label_bytes = n * HW;
  if (overlap({{raw, raw_bytes}}, {{ground, ground_bytes}, {labels, label_bytes}}) || overlap({{ground, ground_bytes}}, {{labels, label_bytes}}))
    return refuse("overlapping buffers");
  using G = sn_handle::Ground;
  G& lane = h->gnd;
  Bracket b(h, "sn_ground_from_raw", mem, stream, lane);
  Staging& s = b.s;
  hipStream_t st = b.c.st;
  const int K = p->hypotheses;
  a.acc_words = 1 + 9 * (p->refits + 1);
  a.raw = s.in_pinned(G::kPinRaw, G::kRaw, raw, raw_bytes);
  a.out = s.out(G::kGround, ground, ground_bytes, true);      // the label pass reads the records
  a.labels = s.out(G::kLabels, labels, label_bytes);
  a.hyp = s.scratch<GrHyp>(G::kHyp, (size_t)n * K * sizeof(GrHyp));
  a.counts = s.scratch<uint32_t>(G::kCounts, (size_t)n * K * 4);
  a.acc = s.scratch<unsigned long long>(G::kAcc, (size_t)n * a.acc_words * 8);
  a.state = s.scratch<GrState>(G::kState, (size_t)n * sizeof(GrState));
  if (s.rc) return s.rc;
  a.W = W, a.H = H, a.step = cam->step, a.n = n;
  a.K = K, a.min_area = p->min_area, a.min_inliers = p->min_inliers, a.refits = p->refits, a.seed = p->seed;
  gr_gate(cam, p, a.roi, kOutScale, a.gate);
  gr_prior(p, a.m);
  a.fx = cam->fx, a.fy = cam->fy, a.cx = cam->cx, a.cy = cam->cy, a.baseline_mm = cam->baseline_mm, a.S = gr_scale(kOutScale);
  {
    const GrFillArgs f{a.counts, a.acc, (size_t)n * K, (size_t)n * a.acc_words};
    hipLaunchKernelGGL(k_gr_fill, dim3((unsigned)std::min<size_t>((f.n_counts + f.n_acc + 255) / 256, 2048)), dim3(256), 0, st, f);
  }
  a.rows = gr_rows(a.roi, K, n);
  const int tiles_x = (a.roi.Ws + 255) / 256;
  const dim3 tiles(tiles_x * ((a.roi.Hs + a.rows - 1) / a.rows), n), tiles8(tiles_x * ((a.roi.Hs + kGrRows - 1) / kGrRows), n), per_map((n + 63) / 64);
  hipLaunchKernelGGL(k_gr_hyp, dim3((K + 255) / 256, n), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_gr_score, tiles, dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_gr_select, dim3(n), dim3(256), 0, st, a);
  for (int round = 0; round <= p->refits; ++round) {
    hipLaunchKernelGGL(k_gr_moments, tiles8, dim3(256), 0, st, a, round);
    if (round < p->refits) hipLaunchKernelGGL(k_gr_solve, per_map, dim3(64), 0, st, a, round);
  }
  hipLaunchKernelGGL(k_gr_finish, per_map, dim3(64), 0, st, a);
  if (a.labels) {
    const dim3 grid((unsigned)std::max<size_t>(1, std::min<size_t>((HW / 4 + 255) / 256, 2048 / n + 1)), n);
    if (!((uintptr_t)a.raw & 15) && !((uintptr_t)a.labels & 3) && HW % 4 == 0) hipLaunchKernelGGL(k_gr_labels<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_gr_labels<false>, grid, dim3(256), 0, st, a);
  }
  HIP_TRY(h, hipGetLastError());
  return b.close();
}

// ---- left-right consistency check (csrc/sn_lrcheck.hpp) --------------------------------------------------------------
int sn_mirror_pair_i8(sn_handle* h, int n, const int8_t* in, int8_t* out, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  const size_t bytes = (size_t)(n > 0 ? n : 0) * 6 * h->H * h->W;
  if (!in || !out || n <= 0 || n > h->max_batch || overlap({{in, bytes}}, {{out, bytes}})) {
    set_err(h, "sn_mirror_pair_i8: bad arguments (in and out must not overlap)");
    return SN_ERR_ARG;
  }
  Bracket b(h, "sn_mirror_pair_i8", mem, stream);
  Staging& s = b.s;
  using S = sn_handle::InferStaging;
  const int8_t* din = s.in(S::kIn, in, bytes);
  int8_t* dout = s.out(S::kMirror, out, bytes);
  if (s.rc) return s.rc;
  if (int rc = mirror_launch(h, b.c.st, n, din, dout)) return rc;
  return b.close();
}

int sn_lr_check(sn_handle* h, int n, const int32_t* raw_left, const int32_t* raw_right, const sn_lrc_params* p,
                int32_t* out_raw, float* disp_inout, uint8_t* mask, uint32_t* kept, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  if (!raw_left || !raw_right || !lrc_params_ok(p) || (!out_raw && !mask) || n <= 0 || n > h->max_batch) {
    set_err(h, "sn_lr_check: bad arguments");
    return SN_ERR_ARG;
  }
  Bracket b(h, "sn_lr_check", mem, stream);
  Staging& s = b.s;
  using S = sn_handle::InferStaging;
  const size_t cnt = (size_t)n * h->H * h->W;
  const int32_t* dl = s.in(S::kLeft, raw_left, cnt * 4);
  const int32_t* dr = s.in(S::kRight, raw_right, cnt * 4);
  int32_t* dout = s.alias(out_raw, s.staged<int32_t>(S::kLeft), cnt * 4);      // host mode: masked in place
  float* ddisp = s.inout(S::kDisp, disp_inout, cnt * 4);
  uint8_t* dmask = s.out(S::kMask, mask, cnt);
  uint32_t* dkept = s.out(S::kKept, kept, (size_t)n * 4);
  if (s.rc) return s.rc;
  if (int rc = lrc_launch(h, b.c.st, n, dl, dr, p, dout, ddisp, dmask, dkept, nullptr)) return rc;
  return b.close();
}

// L = forward(in), M = forward(mirror(in)), then the check of L against M in its mirrored storage: two run_forward calls, so
// each is counted, folded into the refinement statistic and (SN_PREC_AUTO, blocking) repeated by the usual rule.
int sn_infer_lrc(sn_handle* h, int n, const void* in, int in_kind, int w2, int h_px, const sn_lrc_params* p, int32_t* out_i32,
                 float* out_disp, int32_t* out_right_i32, uint8_t* mask, uint32_t* kept, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  if (!in || !lrc_params_ok(p) || (!out_i32 && !out_disp) || n <= 0 || n > h->max_batch) {
    set_err(h, "sn_infer_lrc: bad arguments");
    return SN_ERR_ARG;
  }
  int rc = pair_input_check(h, "sn_infer_lrc", in, in_kind, w2, h_px, mem);
  if (rc) return rc;
  Bracket b(h, "sn_infer_lrc", mem, stream);
  Staging& s = b.s;
  const Call& c = b.c;
  using S = sn_handle::InferStaging;
  const size_t cnt = (size_t)n * h->H * h->W;
  int8_t* dmir = s.scratch<int8_t>(S::kMirror, cnt * 6);
  int32_t* dsecond = s.scratch<int32_t>(S::kRight, cnt * 4);
  int32_t* dleft = s.out(S::kLeft, out_i32, cnt * 4, true);      // the check reads the left map, and masks it in place
  float* ddisp = s.out(S::kDisp, out_disp, cnt * 4);
  int32_t* dright = s.out(S::kRightOut, out_right_i32, cnt * 4);
  uint8_t* dmask = s.out(S::kMask, mask, cnt);
  uint32_t* dkept = s.out(S::kKept, kept, (size_t)n * 4);
  const int8_t* din = pair_input(s, n, in, in_kind, w2, h_px);
  if (s.rc) return s.rc;
  auto nothing = []() -> int { return SN_OK; };
  if ((rc = run_forward(h, c.st, n, din, ddisp, dleft, n == 1, c.blocking, nothing))) return rc;
  if ((rc = mirror_launch(h, c.st, n, din, dmir))) return rc;
  if ((rc = run_forward(h, c.st, n, dmir, nullptr, dsecond, false, c.blocking, nothing))) return rc;
  sn_lrc_params q = *p;
  q.right_mirrored = 1;
  if ((rc = lrc_launch(h, c.st, n, dleft, dsecond, &q, dleft, ddisp, dmask, dkept, dright))) return rc;
  return b.close();
}

// ---- confidence of the soft-argmin distribution and the mask on it (csrc/sn_confidence.hpp) ------------------------------------
// One forward pass whose soft-argmin epilogue also writes the confidence plane; the upsample + mask kernel and the downloads
// are run_forward's `post`, so a call that SN_PREC_AUTO repeats in SN_PREC_F16X3 masks and hands back the repeated maps.
int sn_infer_conf(sn_handle* h, int n, const void* in, int in_kind, int w2, int h_px, const sn_conf_params* p, int32_t* out_i32,
                  float* out_disp, float* out_conf, uint8_t* mask, uint32_t* kept, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  if (!in || (p && !conf_params_ok(p)) || (!p && (mask || kept)) || (!out_i32 && !out_disp) || n <= 0 || n > h->max_batch) {
    set_err(h, "sn_infer_conf: bad arguments");
    return SN_ERR_ARG;
  }
  int rc = pair_input_check(h, "sn_infer_conf", in, in_kind, w2, h_px, mem);
  if (rc) return rc;
  Bracket b(h, "sn_infer_conf", mem, stream);      // opened only: the downloads are in `post`, the sync is run_forward's
  Staging& s = b.s;
  const Call& c = b.c;
  using S = sn_handle::InferStaging;
  const size_t cnt = (size_t)n * h->H * h->W;
  int32_t* draw = s.out(S::kLeft, out_i32, cnt * 4, p != nullptr);      // the mask rules read the map
  float* ddisp = s.out(S::kDisp, out_disp, cnt * 4);
  float* dconf = s.out(S::kConf, out_conf, cnt * 4);
  uint8_t* dmask = s.out(S::kMask, mask, cnt);
  uint32_t* dkept = s.out(S::kKept, kept, (size_t)n * 4);
  const int8_t* din = pair_input(s, n, in, in_kind, w2, h_px);
  if (s.rc) return s.rc;
  auto post = [&]() -> int {
    const int prc = conf_launch(h, c.st, n, true, h->ws.conf_low, draw, p, dconf, draw, ddisp, dmask, dkept);
    return prc ? prc : s.download();
  };
  return run_forward(h, c.st, n, din, ddisp, draw, n == 1, c.blocking, post, true);
}

int sn_conf_mask(sn_handle* h, int n, const int32_t* raw, const float* conf, const sn_conf_params* p, int32_t* out_raw,
                 float* disp_inout, uint8_t* mask, uint32_t* kept, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  if (!raw || !conf || !conf_params_ok(p) || (!out_raw && !mask) || n <= 0 || n > h->max_batch) {
    set_err(h, "sn_conf_mask: bad arguments");
    return SN_ERR_ARG;
  }
  const size_t cnt = (size_t)n * h->H * h->W;
  // conf is read by every pixel's thread: it must not be one of the outputs
  if (overlap({{conf, cnt * 4}}, {{out_raw, cnt * 4}, {disp_inout, cnt * 4}, {mask, cnt}, {kept, (size_t)n * 4}})) {
    set_err(h, "sn_conf_mask: conf overlaps an output");
    return SN_ERR_ARG;
  }
  Bracket b(h, "sn_conf_mask", mem, stream);
  Staging& s = b.s;
  using S = sn_handle::InferStaging;
  const int32_t* draw = s.in(S::kLeft, raw, cnt * 4);
  const float* dconf = s.in(S::kConf, conf, cnt * 4);
  int32_t* dout = s.alias(out_raw, s.staged<int32_t>(S::kLeft), cnt * 4);      // host mode: masked in place
  float* ddisp = s.inout(S::kDisp, disp_inout, cnt * 4);
  uint8_t* dmask = s.out(S::kMask, mask, cnt);
  uint32_t* dkept = s.out(S::kKept, kept, (size_t)n * 4);
  if (s.rc) return s.rc;
  if (int rc = conf_launch(h, b.c.st, n, false, dconf, draw, p, nullptr, dout, ddisp, dmask, dkept)) return rc;
  return b.close();
}

// ---- speckle removal and hole filling (csrc/sn_dispfilter.hpp): a lane of the handle's -----------------------------------------
int sn_filter_raw(sn_handle* h, int n, const int32_t* raw, const sn_filter_params* p, int32_t* out_raw, float* disp_inout,
                  uint8_t* mask, uint32_t* counts, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  const size_t HW = (size_t)h->H * h->W;
  if (!raw || !p || (!out_raw && !mask) || n <= 0 || n > h->max_batch || p->speckle_max_px < 0 ||
      (size_t)p->speckle_max_px > HW || !std::isfinite(p->speckle_diff_px) || p->speckle_diff_px < 0.f || p->fill_max_px < 0 ||
      (p->speckle_max_px == 0 && p->fill_max_px == 0) || HW > 0x7fffffffu) {
    set_err(h, "sn_filter_raw: bad arguments");
    return SN_ERR_ARG;
  }
  const size_t cnt = (size_t)n * HW;
  if (masked_map_overlap(n, HW, raw, out_raw, disp_inout, mask, counts, 3)) {
    set_err(h, "sn_filter_raw: overlapping buffers (only out_raw == raw is allowed)");
    return SN_ERR_ARG;
  }
  using F = sn_handle::Filter;
  Bracket b(h, "sn_filter_raw", mem, stream, h->flt);
  Staging& s = b.s;
  hipStream_t st = b.c.st;
  const int slice = std::min(h->max_batch, kFltSlice);
  uint32_t* scratch = p->speckle_max_px ? s.scratch<uint32_t>(F::kScratch, (size_t)slice * HW * 8) : s.staged<uint32_t>(F::kScratch);
  const float S = (float)((double)kOutScale * kWireFactor);
  const float q = floorf(p->speckle_diff_px / S);
  const int32_t* draw = s.in(F::kRaw, raw, cnt * 4);
  int32_t* dout = s.alias(out_raw, s.staged<int32_t>(F::kRaw), cnt * 4);      // host mode: filtered in place
  float* ddisp = s.inout(F::kDisp, disp_inout, cnt * 4);
  uint8_t* dmask = s.out(F::kMask, mask, cnt);
  uint32_t* dcounts = s.out(F::kCounts, counts, (size_t)n * 12);
  if (s.rc) return s.rc;
  FltArgs a{draw, dout, ddisp, dmask, dcounts, scratch, scratch ? scratch + (size_t)slice * HW : nullptr, h->W, h->H,
            (h->W + kFltTW - 1) / kFltTW, (h->H + kFltTH - 1) / kFltTH, q >= 4294967296.f ? 4294967296ll : (long long)q,
            (uint32_t)p->speckle_max_px, p->fill_max_px, S};
  const FltArgs all = a;
  if (a.counts) HIP_TRY(h, hipMemsetAsync(a.counts, 0, (size_t)n * 12, st));
  const bool vec = (h->W & 3) == 0 && ((uintptr_t)a.mask & 3) == 0;
  const int pairs = (a.tiles_x - 1) * h->H + (a.tiles_y - 1) * h->W;
  for (int k0 = 0; k0 < n; k0 += slice) {      // the scratch holds `slice` maps: walk the batch on the stream
    const int m = std::min(slice, n - k0);
    at_slice(a, all, k0, HW, 3);
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
  return b.close();
}

// ---- guided weighted-median smoothing (csrc/sn_smooth.hpp): a lane of the handle's ------------------------------------------
int sn_smooth_raw(sn_handle* h, int n, const int32_t* raw, const void* guide, int guide_kind, int guide_pitch,
                  const sn_smooth_params* p, int32_t* out_raw, float* disp_inout, uint8_t* mask, uint32_t* counts, int mem,
                  void* stream) {
  if (!h) return SN_ERR_ARG;
  const size_t HW = (size_t)h->H * h->W;
  const bool weighted = p && p->sigma_luma > 0;      // sigma_luma == 0: the guide is ignored altogether
  const GuideSpan g(h, n, guide, guide_kind, guide_pitch, weighted);
  if (!raw || !p || (!out_raw && !mask) || n <= 0 || n > h->max_batch || p->radius < 1 || p->radius > 3 || p->sigma_luma < 0 ||
      p->sigma_luma > 255 || !g.ok || p->min_valid < 0 || p->min_valid > (2 * p->radius + 1) * (2 * p->radius + 1)) {
    set_err(h, "sn_smooth_raw: bad arguments");
    return SN_ERR_ARG;
  }
  const size_t cnt = (size_t)n * HW;
  if (masked_map_overlap(n, HW, raw, out_raw, disp_inout, mask, counts, 3, g.span)) {
    set_err(h, "sn_smooth_raw: overlapping buffers (only out_raw == raw is allowed)");
    return SN_ERR_ARG;
  }
  using M = sn_handle::Smooth;
  Bracket b(h, "sn_smooth_raw", mem, stream, h->smo);
  Staging& s = b.s;
  hipStream_t st = b.c.st;
  const int slice = std::min(h->max_batch, kSmSlice);
  const bool in_place = !s.host && out_raw == raw;      // the kernel reads its neighbours' pixels: it works on a copy
  int32_t* scratch = in_place ? s.scratch<int32_t>(M::kScratch, (size_t)slice * HW * 4) : nullptr;
  const int32_t* draw = s.in(M::kRaw, raw, cnt * 4);
  const uint8_t* dguide = weighted ? s.in(M::kGuide, static_cast<const uint8_t*>(g.span.p), g.span.bytes) : nullptr;
  int32_t* dout = s.out(M::kOut, out_raw, cnt * 4);
  float* ddisp = s.inout(M::kDisp, disp_inout, cnt * 4);
  uint8_t* dmask = s.out(M::kMask, mask, cnt);
  uint32_t* dcounts = s.out(M::kCounts, counts, (size_t)n * 12);
  if (s.rc) return s.rc;
  SmArgs a{draw, dguide, dout, ddisp, dmask, dcounts, g.frame, g.pitch, g.xor_, h->W, h->H,
           (h->W + kSmTW - 1) / kSmTW, p->min_valid, (float)((double)kOutScale * kWireFactor), {}};
  const long long ss = (long long)p->sigma_luma * p->sigma_luma;
  for (int j = 0; j < 256; ++j) a.table[j] = (uint16_t)(weighted ? (256 * ss) / (ss + (long long)j * j) : 1);
  const SmArgs all = a;
  if (a.counts) HIP_TRY(h, hipMemsetAsync(a.counts, 0, (size_t)n * 12, st));
  const int tiles = a.tiles_x * ((h->H + kSmTH - 1) / kSmTH);
  for (int k0 = 0; k0 < n; k0 += slice) {      // the scratch holds `slice` maps: walk the batch on the stream
    const int m = std::min(slice, n - k0);
    at_slice(a, all, k0, HW, 3);
    a.luma = all.luma ? all.luma + (size_t)k0 * g.frame : nullptr;
    if (in_place) {
      HIP_TRY(h, hipMemcpyAsync(scratch, a.raw, (size_t)m * HW * 4, hipMemcpyDeviceToDevice, st));
      a.raw = scratch;
    }
    const dim3 grid(tiles, m), block(256);
    switch (p->radius * 2 + (weighted ? 1 : 0)) {
      case 2: hipLaunchKernelGGL((k_smooth<1, false>), grid, block, 0, st, a); break;
      case 3: hipLaunchKernelGGL((k_smooth<1, true>), grid, block, 0, st, a); break;
      case 4: hipLaunchKernelGGL((k_smooth<2, false>), grid, block, 0, st, a); break;
      case 5: hipLaunchKernelGGL((k_smooth<2, true>), grid, block, 0, st, a); break;
      case 6: hipLaunchKernelGGL((k_smooth<3, false>), grid, block, 0, st, a); break;
      default: hipLaunchKernelGGL((k_smooth<3, true>), grid, block, 0, st, a); break;
    }
  }
  HIP_TRY(h, hipGetLastError());
  return b.close();
}

// ---- temporal filter of disparity streams (csrc/sn_temporal.hpp): an object with its own state and lane ------------------------
int sn_temporal_create(sn_handle* h, int streams, const sn_temporal_params* p, sn_temporal** out) {
  if (!h) return SN_ERR_ARG;
  if (!p || !out || !streams_ok(h, streams) || p->alpha < 1 || p->alpha > 256 || !std::isfinite(p->delta_px) ||
      p->delta_px < 0.f || p->persist < 0 || p->persist > 8 || p->luma_delta < 0 || p->luma_delta > 255) {
    set_err(h, "sn_temporal_create: bad arguments");
    return SN_ERR_ARG;
  }
  std::unique_ptr<sn_temporal> t(new sn_temporal);
  t->p = *p;
  const float q = floorf(p->delta_px / (float)((double)kOutScale * kWireFactor));      // sn_filter_raw's dq
  t->q = q >= 4294967296.f ? 4294967296ll : (long long)q;
  if (const int rc = stream_open(t.get(), h, streams, "sn_temporal_create", &sn_handle::temporal_live,
                                 {{&t->state, (size_t)streams * h->H * h->W * 6}}))
    return rc;
  *out = t.release();
  return SN_OK;
}

int sn_temporal_reset(sn_temporal* t, int stream) { return stream_reset(t, stream, "sn_temporal_reset"); }

void sn_temporal_destroy(sn_temporal* t) { stream_destroy(t, &sn_handle::temporal_live, &sn_temporal::state); }

int sn_temporal_push(sn_temporal* t, int n, const int* stream_of, const int32_t* raw, const void* guide, int guide_kind,
                     int guide_pitch, int32_t* out_raw, float* disp_inout, uint8_t* mask, uint32_t* counts, int mem,
                     void* stream) {
  if (!t) return SN_ERR_ARG;
  sn_handle* h = t->h;
  const size_t HW = (size_t)h->H * h->W;
  const bool luma = t->p.luma_delta > 0;      // luma_delta == 0: the guide is ignored altogether
  const GuideSpan g(h, n, guide, guide_kind, guide_pitch, luma);
  bool ok = raw && (out_raw || mask) && n > 0 && n <= h->max_batch && g.ok;
  for (int k = 0; ok && stream_of && k < n; ++k) ok = stream_of[k] >= 0 && stream_of[k] < t->streams;
  if (!ok) {
    set_err(h, "sn_temporal_push: bad arguments");
    return SN_ERR_ARG;
  }
  const size_t cnt = (size_t)n * HW;
  if (masked_map_overlap(n, HW, raw, out_raw, disp_inout, mask, counts, 4, g.span)) {
    set_err(h, "sn_temporal_push: overlapping buffers (only out_raw == raw is allowed)");
    return SN_ERR_ARG;
  }
  using T = sn_temporal;
  Bracket b(h, "sn_temporal_push", mem, stream, *t);      // the wait: the previous push (any stream) is done with the state too
  Staging& s = b.s;
  hipStream_t st = b.c.st;
  const int32_t* draw = s.in(T::kRaw, raw, cnt * 4);
  const uint8_t* dguide = luma ? s.in(T::kGuide, static_cast<const uint8_t*>(g.span.p), g.span.bytes) : nullptr;
  int32_t* dout = s.alias(out_raw, s.staged<int32_t>(T::kRaw), cnt * 4);      // host mode: filtered in place
  float* ddisp = s.inout(T::kDisp, disp_inout, cnt * 4);
  uint8_t* dmask = s.out(T::kMask, mask, cnt);
  uint32_t* dcounts = s.out(T::kCounts, counts, (size_t)n * 16);
  if (s.rc) return s.rc;
  int32_t* P = static_cast<int32_t*>(t->state);
  uint8_t* Hs = reinterpret_cast<uint8_t*>(P + (size_t)t->streams * HW);
  TmpArgs a{};
  a.raw = draw, a.luma = dguide, a.out_raw = dout, a.disp = ddisp, a.mask = dmask, a.counts = dcounts;
  a.P = P, a.Hs = Hs, a.Yp = Hs + (size_t)t->streams * HW;
  a.luma_frame = g.frame, a.luma_pitch = g.pitch, a.luma_xor = g.xor_;
  a.W = h->W, a.H = h->H, a.alpha = t->p.alpha, a.persist = t->p.persist, a.luma_delta = t->p.luma_delta, a.q = t->q;
  a.S = (float)((double)kOutScale * kWireFactor);
  if (dcounts) HIP_TRY(h, hipMemsetAsync(dcounts, 0, (size_t)n * 16, st));
  // 16-byte map accesses, 4-byte luma and mask accesses: every address the kernel forms must be that aligned
  const bool vec = (h->W & 3) == 0 && (((uintptr_t)draw | (uintptr_t)dout) & 15) == 0 && ((uintptr_t)dmask & 3) == 0 &&
                   (!luma || (((uintptr_t)dguide | g.frame | (size_t)g.pitch) & 3) == 0);
  const unsigned chunks = (unsigned)((HW + (vec ? 1023 : 255)) / (vec ? 1024 : 256));
  const TmpArgs all = a;
  for (int k0 = 0; k0 < n; k0 += kSlice) {      // the frame lists of kSlice maps fit the kernel arguments
    const int m = std::min(kSlice, n - k0);
    at_slice(a, all, k0, HW, 4);
    a.luma = all.luma ? all.luma + (size_t)k0 * g.frame : nullptr;
    int last[kSlice];      // per group: its last map of the slice (the filter keeps nothing of it)
    const int groups = group_slice(a.g, last, stream_of, k0, m, t->fresh.data());
    const dim3 grid(chunks, groups), block(256);
    switch ((vec ? 2 : 0) + (luma ? 1 : 0)) {
      case 0: hipLaunchKernelGGL((k_temporal<false, false>), grid, block, 0, st, a); break;
      case 1: hipLaunchKernelGGL((k_temporal<false, true>), grid, block, 0, st, a); break;
      case 2: hipLaunchKernelGGL((k_temporal<true, false>), grid, block, 0, st, a); break;
      default: hipLaunchKernelGGL((k_temporal<true, true>), grid, block, 0, st, a); break;
    }
    HIP_TRY(h, hipGetLastError());
    commit_slice(a.g, groups, t->fresh.data());
  }
  return b.close();
}

// ---- JPEG of NV12 images (csrc/sn_jpeg.hpp): a lane of the handle's -------------------------------------------------------------
size_t sn_jpeg_bound(int w, int h_px) { return jpg_bound(w, h_px); }

int sn_jpeg_encode_nv12(sn_handle* h, int n, const uint8_t* nv12, int w, int h_px, int pitch, size_t frame, const sn_jpeg_params* p,
                        uint8_t* out, size_t out_stride, uint32_t* sizes, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  auto bad = [&](const char* why) {
    set_err(h, std::string("sn_jpeg_encode_nv12: ") + why);
    return SN_ERR_ARG;
  };
  if (!nv12 || !p || !out || !sizes || n <= 0 || n > h->max_batch) return bad("bad arguments");
  if (!jpg_size_ok(w, h_px)) return bad("the width and the height must be even and within 2..65535");
  if (pitch < w) return bad("pitch < w");
  const long long restart = jpg_restart_mcus(w, h_px, p->rows_per_slice);
  if (restart > 65535) return bad("more than 65535 MCUs per restart interval");
  const size_t bound = jpg_bound(w, h_px);
  if (bound > 0xffffffffu) return bad("the image is too large: a stream could exceed 2^32 bytes");
  const size_t span = (size_t)(n - 1) * frame + (size_t)(h_px + h_px / 2 - 1) * pitch + w;
  {
    const Span in{nv12, span}, o{out, n * out_stride}, z{sizes, (size_t)n * 4};
    if (overlap({in}, {o, z}) || overlap({o}, {z})) return bad("overlapping buffers");
  }
  using J = sn_handle::JpegSlots;
  Bracket b(h, "sn_jpeg_encode_nv12", mem, stream, h->jpg);
  Staging& s = b.s;
  const uint8_t* din = s.in(J::kIn, nv12, span);
  if (s.rc) return s.rc;
  auto source = [&](int k0, int, const uint8_t** src) {
    *src = din + (size_t)k0 * frame;
    return SN_OK;
  };
  if (int rc = jpeg_walk(h, s, b.c.st, h->jpg.plan, JpgSlotIds{J::kCoef, J::kBytes, J::kLens, J::kOut, J::kSizes}, n, w, h_px, pitch,
                         frame, p, (int)restart, out, out_stride, sizes, source))
    return rc;
  return b.close();
}

// ---- the depth view (csrc/sn_render.hpp): a lane of the handle's ------------------------------------------------------------------
int sn_render_tables(const sn_render_params* p, uint8_t* rgb, uint8_t* ycc) {
  return render_tables(p, rgb, ycc) ? SN_OK : SN_ERR_ARG;
}

int sn_render(sn_handle* h, int n, const int32_t* raw, const uint8_t* left_nv12, int left_pitch, const sn_render_params* p, int format,
              uint8_t* out, int out_pitch, size_t out_frame, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  auto bad = [&](const char* why) {
    set_err(h, std::string("sn_render: ") + why);
    return SN_ERR_ARG;
  };
  RenderCall c;
  if (const char* why = render_check(h, n, raw, left_nv12, left_pitch, p, format, &c)) return bad(why);
  if (!out) return bad("a NULL pointer");
  if (out_pitch < c.row_bytes) return bad("out_pitch is smaller than a row of the canvas");
  const size_t canvas = (size_t)(c.rows - 1) * out_pitch + c.row_bytes;
  if (out_frame < canvas) return bad("out_frame is smaller than a canvas");
  if (overlap({{out, (n - 1) * out_frame + canvas}}, {{raw, c.raw_bytes}, {c.stack ? left_nv12 : nullptr, c.left_span}}))
    return bad("out overlaps an input");
  using R = sn_handle::RenderSlots;
  Bracket b(h, "sn_render", mem, stream, h->rnd);
  Staging& s = b.s;
  hipStream_t st = b.c.st;
  const int32_t* draw = s.in(R::kRaw, raw, c.raw_bytes);
  const uint8_t* dleft = c.stack ? s.in(R::kLeft, left_nv12, c.left_span) : nullptr;
  // host mode: the canvases are staged at their minimal pitch and copied back row by row, so the caller's padding stays untouched
  const size_t tight = (size_t)c.rows * c.row_bytes;
  uint8_t* dout = s.host ? s.scratch<uint8_t>(R::kOut, n * tight) : out;
  if (s.rc) return s.rc;
  if (int rc = render_launch(h, st, n, c, draw, dleft, left_pitch, dout, s.host ? c.row_bytes : out_pitch, s.host ? tight : out_frame))
    return rc;
  for (int k = 0; s.host && k < n; ++k)
    HIP_TRY(h, hipMemcpy2DAsync(out + k * out_frame, out_pitch, dout + k * tight, c.row_bytes, c.row_bytes, c.rows,
                                hipMemcpyDeviceToHost, st));
  return b.close();
}

int sn_render_jpeg(sn_handle* h, int n, const int32_t* raw, const uint8_t* left_nv12, int left_pitch, const sn_render_params* p,
                   const sn_jpeg_params* jp, uint8_t* out, size_t out_stride, uint32_t* sizes, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  auto bad = [&](const char* why) {
    set_err(h, std::string("sn_render_jpeg: ") + why);
    return SN_ERR_ARG;
  };
  RenderCall c;
  if (const char* why = render_check(h, n, raw, left_nv12, left_pitch, p, SN_RENDER_NV12, &c)) return bad(why);
  if (!jp || !out || !sizes) return bad("a NULL pointer");
  const int W = h->W;
  if (!jpg_size_ok(W, c.Hc)) return bad("the canvas must be within 2..65535 pixels a side");
  const long long restart = jpg_restart_mcus(W, c.Hc, jp->rows_per_slice);
  if (restart > 65535) return bad("more than 65535 MCUs per restart interval");
  if (jpg_bound(W, c.Hc) > 0xffffffffu) return bad("the canvas is too large: a stream could exceed 2^32 bytes");
  {
    const Span o{out, n * out_stride}, z{sizes, (size_t)n * 4};
    if (overlap({o}, {{raw, c.raw_bytes}, {c.stack ? left_nv12 : nullptr, c.left_span}, z}) ||
        overlap({z}, {{raw, c.raw_bytes}, {c.stack ? left_nv12 : nullptr, c.left_span}}))
      return bad("out or sizes overlaps another buffer");
  }
  using R = sn_handle::RenderSlots;
  Bracket b(h, "sn_render_jpeg", mem, stream, h->rnd);
  Staging& s = b.s;
  hipStream_t st = b.c.st;
  const size_t HW = (size_t)h->H * W, frame = (size_t)c.rows * W;      // the canvas at pitch W
  const int32_t* draw = s.in(R::kRaw, raw, c.raw_bytes);
  const uint8_t* dleft = c.stack ? s.in(R::kLeft, left_nv12, c.left_span) : nullptr;
  uint8_t* canvas = s.scratch<uint8_t>(R::kCanvas, std::min(h->max_batch, kJpgSlice) * frame);
  if (s.rc) return s.rc;
  auto source = [&](int k0, int m, const uint8_t** src) {
    *src = canvas;
    return render_launch(h, st, m, c, draw + k0 * HW, dleft ? dleft + k0 * c.left_frame : nullptr, left_pitch, canvas, W, frame);
  };
  if (int rc = jpeg_walk(h, s, st, h->rnd.plan, JpgSlotIds{R::kCoef, R::kBytes, R::kLens, R::kJpegOut, R::kSizes}, n, W, c.Hc, W,
                         frame, jp, (int)restart, out, out_stride, sizes, source))
    return rc;
  return b.close();
}

// ---- stereo rectification (csrc/sn_rectify.hpp): an object with its own maps and lane -----------------------------------------
int sn_rectify_build_map(const sn_stereo_calib* c, int eye, int w, int h_px, int32_t* map_xy) {
  if (!rect_calib_ok(c) || !map_xy || (eye != 0 && eye != 1) || w < 1 || h_px < 1) return SN_ERR_ARG;
  rectify_build_map(*c, eye, w, h_px, map_xy);
  return SN_OK;
}

int sn_rectify_create(sn_handle* h, const sn_stereo_calib* c, sn_rectify** out) {
  if (!h) return SN_ERR_ARG;
  if (!out || !rect_calib_ok(c)) {
    set_err(h, "sn_rectify_create: bad arguments");
    return SN_ERR_ARG;
  }
  if ((h->W & 3) || (h->H & 1)) {
    set_err(h, "sn_rectify_create: the model's width must be a multiple of 4 and its height even");
    return SN_ERR_ARG;
  }
  const int rc = check_device(h);
  if (rc) return rc;
  const size_t words = (size_t)h->H * h->W * 2;
  std::vector<int32_t> maps;
  try {
    maps.resize(2 * words);
  } catch (const std::bad_alloc&) {
    set_err(h, "sn_rectify_create: out of memory");
    return SN_ERR_NOMEM;
  }
  std::unique_ptr<sn_rectify> r(new sn_rectify);
  r->h = h;
  r->c = *c;
  for (int eye = 0; eye < 2; ++eye) r->valid[eye] = rectify_build_map(*c, eye, h->W, h->H, maps.data() + eye * words);
  if (hipMalloc(&r->map, 2 * words * 4) != hipSuccess) {
    (void)hipGetLastError();
    set_err(h, "sn_rectify_create: out of device memory");
    return SN_ERR_NOMEM;
  }
  if (hipMemcpy(r->map, maps.data(), 2 * words * 4, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(r->map);
    set_err(h, "sn_rectify_create: the upload of the maps failed");
    return SN_ERR_DEVICE;
  }
  ++h->rectify_live;
  *out = r.release();
  return SN_OK;
}

void sn_rectify_destroy(sn_rectify* r) {
  if (!r) return;
  (void)hipSetDevice(r->h->device);
  r->destroy();
  (void)hipFree(r->map);
  --r->h->rectify_live;
  delete r;
}

int sn_rectify_get_info(const sn_rectify* r, sn_rectify_info* info) {
  if (!r || !info) return SN_ERR_ARG;
  *info = sn_rectify_info{r->c.src_w, r->c.src_h, r->h->W, r->h->H, r->valid[0], r->valid[1]};
  return SN_OK;
}

int sn_rectify_get_camera(const sn_rectify* r, sn_camera* cam) {
  if (!r || !cam) return SN_ERR_ARG;
  *cam = sn_camera{(float)r->c.pfx, (float)r->c.pfy, (float)r->c.pcx, (float)r->c.pcy, (float)r->c.baseline_mm, 0.f, 0.f, 1};
  return SN_OK;
}

int sn_rectify_get_map(sn_rectify* r, int eye, int32_t* map_xy_host) {
  if (!r) return SN_ERR_ARG;
  sn_handle* h = r->h;
  if (!map_xy_host || (eye != 0 && eye != 1)) {
    set_err(h, "sn_rectify_get_map: bad arguments");
    return SN_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(r->mu);
  const int rc = check_device(h);
  if (rc) return rc;
  const size_t words = (size_t)h->H * h->W * 2;
  HIP_TRY(h, hipMemcpy(map_xy_host, r->map + eye * words, words * 4, hipMemcpyDeviceToHost));
  return SN_OK;
}

int sn_rectify_nv12(sn_rectify* r, int n, const uint8_t* left, const uint8_t* right, int src_pitch, size_t src_frame,
                    uint8_t* out_sbs_nv12, int8_t* out_nchw6, int mem, void* stream) {
  if (!r) return SN_ERR_ARG;
  sn_handle* h = r->h;
  const int sw = r->c.src_w, sh = r->c.src_h, rows = sh + sh / 2;
  if (!left || !right || (!out_sbs_nv12 && !out_nchw6) || n <= 0 || n > h->max_batch || src_pitch < sw ||
      (size_t)src_pitch * rows > 0x7fffffffu) {
    set_err(h, "sn_rectify_nv12: bad arguments");
    return SN_ERR_ARG;
  }
  if (mem == SN_MEM_DEVICE && (((uintptr_t)out_sbs_nv12 | (uintptr_t)out_nchw6) & 3)) {
    set_err(h, "sn_rectify_nv12: device outputs must be 4-byte aligned");
    return SN_ERR_ARG;
  }
  const size_t HW = (size_t)h->H * h->W;
  // an eye's span: from its first byte to the last byte of the last chroma row of pair n - 1
  const size_t span = (size_t)(n - 1) * src_frame + (size_t)(rows - 1) * src_pitch + sw;
  {
    const Span l{left, span}, rr{right, span}, o{out_sbs_nv12, n * 3 * HW}, t{out_nchw6, n * 6 * HW};
    if (overlap({l, rr}, {o, t}) || overlap({o}, {t})) {
      set_err(h, "sn_rectify_nv12: overlapping buffers (an input and an output, or the two outputs)");
      return SN_ERR_ARG;
    }
  }
  using R = sn_rectify;
  Bracket b(h, "sn_rectify_nv12", mem, stream, *r);
  Staging& s = b.s;
  hipStream_t st = b.c.st;
  const uint8_t *dl = left, *dr = right;
  if (s.host) {
    // a side-by-side frame's eyes share their rows: one upload from the lower address, and both eyes keep their offsets
    const uint8_t *lo = left < right ? left : right, *hi = left < right ? right : left;
    if ((size_t)(hi - lo) < span) {
      const uint8_t* d = s.in(R::kLeft, lo, (size_t)(hi - lo) + span);
      dl = d ? d + (left - lo) : nullptr;
      dr = d ? d + (right - lo) : nullptr;
    } else {
      dl = s.in(R::kLeft, left, span);
      dr = s.in(R::kRight, right, span);
    }
  }
  uint8_t* dsbs = s.out(R::kSbs, out_sbs_nv12, n * 3 * HW, out_nchw6 != nullptr);      // k_pre_nv12 reads the rectified frame
  int8_t* dten = s.out(R::kTensor, out_nchw6, n * 6 * HW);
  if (s.rc) return s.rc;
  RectArgs a{{dl, dr}, r->map, dsbs, src_frame, src_pitch, sw, sh, h->W, h->H, n};
  const int items = (h->H + h->H / 2) * (h->W / 4);
  hipLaunchKernelGGL(k_rectify, dim3((items + 255) / 256, 2), dim3(256), 0, st, a);
  HIP_TRY(h, hipGetLastError());
  if (dten) {
    const int e = sbs_to_tensors(h, st, n, dsbs, 2 * h->W, h->H, false, dten);
    if (e) return e;
  }
  return b.close();
}

// ---- rolling log-odds costmap (csrc/sn_costmap.hpp): an object with its own state and lane ----------------------------------------
namespace {
// llrint(v) for a finite v, values beyond +-lim taken as +-lim
long long cm_llrint_sat(double v, double lim) { return v >= lim ? (long long)lim : (v <= -lim ? -(long long)lim : std::llrint(v)); }
}  // namespace

int sn_costmap_create(sn_handle* h, int streams, const sn_obstacle_params* op, const sn_costmap_params* p, sn_costmap** out) {
  auto refuse = [&](const char* why) {
    set_err(h, std::string("sn_costmap_create: ") + why);
    return SN_ERR_ARG;
  };
  if (!op || !p || !out) return refuse("a NULL pointer");
  if (!streams_ok(h, streams)) return refuse("streams must be 1..max_batch");
  if (p->mw < 1 || p->mh < 1 || p->mw > kCmMaxWindow || p->mh > kCmMaxWindow) return refuse("mw and mh must be 1..4096");
  if (p->l_hit < 1 || p->l_hit > 32767 || p->l_miss < 1 || p->l_miss > 32767) return refuse("l_hit and l_miss must be 1..32767");
  if (!(p->l_min >= -32767 && p->l_min < 0 && p->l_max > 0 && p->l_max <= 32767)) return refuse("-32767 <= l_min < 0 < l_max <= 32767 is required");
  for (float v : {p->clear_margin_m, p->clear_min_m, p->clear_max_m, op->cell_m, op->x_min_m, op->y_min_m})
    if (!std::isfinite(v)) return refuse("every parameter must be finite");
  if (p->clear_margin_m < 0.f || p->clear_min_m < 0.f || p->clear_max_m < 0.f) return refuse("the clear_* distances must not be negative");
  if (!(op->cell_m > 0.f)) return refuse("cell_m must be positive");
  if (op->gw < 0 || op->gh < 0 || op->gw > kObMaxCells || op->gh > kObMaxCells || (op->gw == 0) != (op->gh == 0))
    return refuse("gw and gh must be 1..4096, or both 0");
  if (op->beams < 0 || op->beams > kObMaxBeams) return refuse("beams must be 0..4096");
  if (op->gw == 0 && op->beams == 0) return refuse("neither a grid nor a scan");
  std::vector<float> edges(op->beams + 1);
  if (op->beams > 0 && !ob_beam_edges(op->beams, op->angle_min_rad, op->angle_increment_rad, edges.data()))
    return refuse("the scan's sector must lie inside (-pi/2, pi/2) with increasing edges");
  std::unique_ptr<sn_costmap> c(new sn_costmap);
  c->p = *p;
  c->gw = op->gw, c->gh = op->gh, c->beams = op->beams;
  c->k256 = 256.0 / (double)op->cell_m;
  const double far = 1099511627776.0, cap = 2147483648.0;      // 2^40, 2^31
  c->gx0 = cm_llrint_sat((double)op->x_min_m / (double)op->cell_m * 256.0, far);
  c->gy0 = cm_llrint_sat((double)op->y_min_m / (double)op->cell_m * 256.0, far);
  c->margin = cm_llrint_sat((double)p->clear_margin_m * c->k256, cap);
  c->rmin = cm_llrint_sat((double)p->clear_min_m * c->k256, cap);
  c->cmax = cm_llrint_sat((double)p->clear_max_m * c->k256, cap);
  // without a handle: a host-only object for sn_costmap_pose_q
  if (const int rc = stream_open(c.get(), h, streams, "sn_costmap_create", &sn_handle::costmap_live,
                                 {{reinterpret_cast<void**>(&c->state), (size_t)streams * p->mw * p->mh * 2},
                                  {reinterpret_cast<void**>(&c->edges), edges.size() * 4}}))
    return rc;
  if (h && hipMemcpy(c->edges, edges.data(), edges.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    sn_costmap_destroy(c.release());
    set_err(h, "sn_costmap_create: the upload of the beam table failed");
    return SN_ERR_DEVICE;
  }
  *out = c.release();
  return SN_OK;
}

int sn_costmap_reset(sn_costmap* c, int stream) { return stream_reset(c, stream, "sn_costmap_reset"); }

void sn_costmap_destroy(sn_costmap* c) { stream_destroy(c, &sn_handle::costmap_live, &sn_costmap::state, &sn_costmap::edges); }

int sn_costmap_pose_q(const sn_costmap* c, const double pose[3], int32_t q[6]) {
  return c && pose && q && torus_pose_q(c, pose, q) ? SN_OK : SN_ERR_ARG;
}

int sn_costmap_push(sn_costmap* c, int n, const int* stream_of, const double* poses, const int8_t* occ, const float* ranges,
                    int8_t* grid, int16_t* logodds, uint32_t* stats, int32_t* pose_q_out, int mem, void* stream) {
  if (!c || !c->h) return SN_ERR_ARG;
  sn_handle* h = c->h;
  auto refuse = [&](const char* why) {
    set_err(h, std::string("sn_costmap_push: ") + why);
    return SN_ERR_ARG;
  };
  if (n <= 0 || n > h->max_batch || !poses) return refuse("bad arguments");
  if (c->gw == 0) occ = nullptr;
  if (c->beams == 0) ranges = nullptr;
  if (!occ && !ranges) return refuse("neither occ nor ranges");
  if (!grid && !logodds && !stats) return refuse("no output");
  for (int k = 0; stream_of && k < n; ++k)
    if (stream_of[k] < 0 || stream_of[k] >= c->streams) return refuse("a stream id out of range");
  if (((uintptr_t)logodds & 1) || ((uintptr_t)stats & 3) || ((uintptr_t)ranges & 3)) return refuse("a misaligned buffer");
  std::vector<int32_t> q((size_t)n * 6);
  for (int k = 0; k < n; ++k)
    if (!torus_pose_q(c, poses + 3 * k, q.data() + 6 * k)) return refuse("a pose that is not finite or too far from the origin");
  const size_t cells = (size_t)c->p.mw * c->p.mh, ocells = (size_t)c->gw * c->gh;
  {
    const Span i0{occ, n * ocells}, i1{ranges, (size_t)n * c->beams * 4}, o0{grid, n * cells}, o1{logodds, n * cells * 2},
        o2{stats, (size_t)n * 16};
    if (overlap({i0, i1}, {o0, o1, o2}) || overlap({o0}, {o1, o2}) || overlap({o1}, {o2})) return refuse("overlapping buffers");
  }
  using T = sn_costmap;
  Bracket b(h, "sn_costmap_push", mem, stream, *c);      // the wait: the previous push (any stream) is done with the state too
  Staging& s = b.s;
  hipStream_t st = b.c.st;
  const int8_t* docc = occ ? s.in(T::kOcc, occ, n * ocells) : nullptr;
  const float* dranges = ranges ? s.in(T::kRanges, ranges, (size_t)n * c->beams * 4) : nullptr;
  int8_t* dgrid = s.out(T::kGrid, grid, n * cells);
  int16_t* dlog = s.out(T::kLog, logodds, n * cells * 2);
  uint32_t* dstats = s.out(T::kStats, stats, (size_t)n * 16);
  if (s.rc) return s.rc;
  if (pose_q_out) memcpy(pose_q_out, q.data(), q.size() * 4);
  CmArgs a{};
  a.edges = c->edges, a.L = c->state, a.k256 = c->k256;
  a.gx0 = c->gx0, a.gy0 = c->gy0, a.margin = c->margin, a.rmin = c->rmin, a.cmax = c->cmax;
  a.mw = c->p.mw, a.mh = c->p.mh, a.gw = c->gw, a.gh = c->gh, a.beams = c->beams;
  a.l_hit = c->p.l_hit, a.l_miss = c->p.l_miss, a.l_min = c->p.l_min, a.l_max = c->p.l_max;
  if (dstats) HIP_TRY(h, hipMemsetAsync(dstats, 0, (size_t)n * 16, st));
  const unsigned chunks = (unsigned)((cells + 255) / 256);
  const size_t lds = dranges ? (size_t)(3 * c->beams + 1) * 4 : 0;      // E, and Rb twice
  for (int k0 = 0; k0 < n; k0 += kSlice) {      // the frame lists and the poses of kSlice maps fit the kernel arguments
    const int m = std::min(kSlice, n - k0);
    a.occ = docc ? docc + k0 * ocells : nullptr;
    a.ranges = dranges ? dranges + (size_t)k0 * c->beams : nullptr;
    a.grid = dgrid ? dgrid + k0 * cells : nullptr;
    a.logodds = dlog ? dlog + k0 * cells : nullptr;
    a.stats = dstats ? dstats + (size_t)k0 * 4 : nullptr;
    memcpy(a.q, q.data() + (size_t)k0 * 6, (size_t)m * 24);
    int last[kSlice];      // per group: its last map of the slice
    const int groups = group_slice(a.g, a.t, last, stream_of, k0, m, c->fresh.data(), c->ox.data(), c->oy.data());
    hipLaunchKernelGGL(k_costmap, dim3(chunks, groups), dim3(256), lds, st, a);
    HIP_TRY(h, hipGetLastError());
    commit_slice(a.g, groups, last, a.q, c->fresh.data(), c->ox.data(), c->oy.data());
  }
  return b.close();
}

// ---- rolling elevation map and traversability (csrc/sn_elevation.hpp): an object with its own state and lane, as the costmap ----
namespace {
// (int)floorf(v * 1000.f) for |v| <= 32
int el_mm(float v) {
  volatile float prod = v * 1000.f;      // one rounded fp32 product
  return (int)std::floor(prod);
}
}  // namespace

int sn_elevation_create(sn_handle* h, int streams, const sn_elevation_params* p, sn_elevation** out) {
  auto refuse = [&](const char* why) {
    set_err(h, std::string("sn_elevation_create: ") + why);
    return SN_ERR_ARG;
  };
  if (!p || !out) return refuse("a NULL pointer");
  if (!streams_ok(h, streams)) return refuse("streams must be 1..max_batch");
  if (p->mw < 1 || p->mh < 1 || p->mw > kElMaxWindow || p->mh > kElMaxWindow) return refuse("mw and mh must be 1..4096");
  for (float v : p->base_from_cam)
    if (!std::isfinite(v)) return refuse("base_from_cam must be finite");
  for (float v : {p->cell_m, p->z_min_m, p->z_max_m, p->range_max_m})
    if (!std::isfinite(v)) return refuse("every parameter must be finite");
  if (!(p->cell_m > 0.f)) return refuse("cell_m must be positive");
  if (p->z_min_m < -32.f || p->z_max_m > 32.f || p->z_min_m > p->z_max_m) return refuse("-32 <= z_min_m <= z_max_m <= 32 is required");
  if (!(p->range_max_m > 0.f)) return refuse("range_max_m must be positive");
  if (p->min_points < 1) return refuse("min_points must be at least 1");
  if (p->alpha < 1 || p->alpha > 256) return refuse("alpha must be 1..256");
  if (p->max_step_mm < 1 || p->max_step_mm > 32767) return refuse("max_step_mm must be 1..32767");
  if (p->radius < 1 || p->radius > kElMaxRadius) return refuse("radius must be 1..3");
  if (p->flags != 0) return refuse("flags must be 0");
  std::unique_ptr<sn_elevation> e(new sn_elevation);
  e->p = *p;
  e->k256 = 256.0 / (double)p->cell_m;
  e->zmin_mm = el_mm(p->z_min_m), e->zmax_mm = el_mm(p->z_max_m);
  // without a handle: a host-only object for sn_elevation_pose_q
  if (const int rc = stream_open(e.get(), h, streams, "sn_elevation_create", &sn_handle::elevation_live,
                                 {{reinterpret_cast<void**>(&e->state), (size_t)streams * p->mw * p->mh * 4}}))
    return rc;
  *out = e.release();
  return SN_OK;
}

int sn_elevation_reset(sn_elevation* e, int stream) { return stream_reset(e, stream, "sn_elevation_reset"); }

void sn_elevation_destroy(sn_elevation* e) { stream_destroy(e, &sn_handle::elevation_live, &sn_elevation::state); }

int sn_elevation_pose_q(const sn_elevation* e, const double pose[3], int32_t q[6]) {
  return e && pose && q && torus_pose_q(e, pose, q) ? SN_OK : SN_ERR_ARG;
}

int sn_elevation_push(sn_elevation* e, int n, const int* stream_of, const double* poses, const int32_t* raw, const sn_camera* cam,
                      const float* mounts, int mount_stride, int8_t* trav, int16_t* hi, int16_t* lo, uint16_t* rise, uint32_t* stats,
                      int32_t* pose_q_out, int mem, void* stream) {
  if (!e || !e->h) return SN_ERR_ARG;
  sn_handle* h = e->h;
  auto refuse = [&](const char* why) {
    set_err(h, std::string("sn_elevation_push: ") + why);
    return SN_ERR_ARG;
  };
  if (n <= 0 || n > h->max_batch || !poses || !raw) return refuse("bad arguments");
  if (!camera_ok(cam)) return refuse("a camera sn_pointcloud_from_raw refuses");
  if (!trav && !hi && !lo && !rise && !stats) return refuse("no output");
  for (int k = 0; stream_of && k < n; ++k)
    if (stream_of[k] < 0 || stream_of[k] >= e->streams) return refuse("a stream id out of range");
  if (((uintptr_t)raw & 3) || ((uintptr_t)stats & 3) || ((uintptr_t)mounts & 3) || ((uintptr_t)hi & 1) || ((uintptr_t)lo & 1) ||
      ((uintptr_t)rise & 1))
    return refuse("a misaligned buffer");
  if (mounts && mount_stride < 12) return refuse("mount_stride must be at least 12");
  std::vector<int32_t> q((size_t)n * 6);
  for (int k = 0; k < n; ++k)
    if (!torus_pose_q(e, poses + 3 * k, q.data() + 6 * k)) return refuse("a pose that is not finite or too far from the origin");
  const int W = h->W, H = h->H, step = cam->step;
  const int Wo = (W + step - 1) / step, Ho = (H + step - 1) / step;
  const size_t cells = (size_t)e->p.mw * e->p.mh, raw_bytes = (size_t)n * H * W * 4;
  const size_t mounts_bytes = mounts ? ((size_t)(n - 1) * mount_stride + 12) * 4 : 0;
  {
    const Span in[2] = {{raw, raw_bytes}, {mounts, mounts_bytes}};
    const Span o[5] = {{trav, n * cells}, {hi, n * cells * 2}, {lo, n * cells * 2}, {rise, n * cells * 2}, {stats, (size_t)n * 16}};
    for (int a = 0; a < 5; ++a) {
      if (overlap({in[0], in[1]}, {o[a]})) return refuse("overlapping buffers");
      for (int b = a + 1; b < 5; ++b)
        if (overlap({o[a]}, {o[b]})) return refuse("overlapping buffers");
    }
  }
  using T = sn_elevation;
  Bracket b(h, "sn_elevation_push", mem, stream, *e);      // the wait: the previous push (any stream) is done with the state too
  Staging& s = b.s;
  hipStream_t st = b.c.st;
  const int32_t* draw = s.in_pinned(T::kPinRaw, T::kRaw, raw, raw_bytes);
  std::vector<float> packed;      // host mode: the mounts, twelve a map (the call is blocking, so it outlives the copy)
  const float* dmounts = mounts;
  if (mounts && s.host) {
    packed.resize((size_t)n * 12);
    for (int k = 0; k < n; ++k) memcpy(&packed[(size_t)k * 12], mounts + (size_t)k * mount_stride, 48);
    dmounts = s.in(T::kMounts, packed.data(), packed.size() * 4);
  }
  const int dstride = mounts && s.host ? 12 : mount_stride;
  int8_t* dtrav = s.out(T::kTrav, trav, n * cells);
  uint16_t* drise = s.out(T::kRise, rise, n * cells * 2);
  uint32_t* dstats = s.out(T::kStats, stats, (size_t)n * 16);
  // the verdict reads the unrolled planes: where the caller takes one, that is the plane; otherwise the scratch (in host mode
  // a caller's plane is the staged copy that is downloaded)
  int16_t* dhi = hi ? s.out(T::kHi, hi, n * cells * 2) : nullptr;
  int16_t* dlo = lo ? s.out(T::kLo, lo, n * cells * 2) : nullptr;
  if (!dhi || !dlo) {
    int16_t* planes = s.scratch<int16_t>(T::kPlanes, n * cells * 4);
    if (planes && !dhi) dhi = planes;
    if (planes && !dlo) dlo = planes + n * cells;
  }
  uint32_t* acc = s.scratch<uint32_t>(T::kAcc, n * cells * 12);
  if (s.rc) return s.rc;
  if (pose_q_out) memcpy(pose_q_out, q.data(), q.size() * 4);
  uint32_t* dcnt = acc;
  int32_t* dfmax = reinterpret_cast<int32_t*>(acc + n * cells);
  int32_t* dfmin = reinterpret_cast<int32_t*>(acc + 2 * n * cells);
  {
    const ElClearArgs c{dcnt, dfmax, dfmin, dstats, n * cells, dstats ? (size_t)n * 4 : 0};
    hipLaunchKernelGGL(k_el_clear, dim3((unsigned)std::min<size_t>((n * cells + 255) / 256, 2048)), dim3(256), 0, st, c);
  }
  ElScatterArgs sa{};
  sa.pc.W = W, sa.pc.H = H, sa.pc.Wo = Wo, sa.pc.Ho = Ho, sa.pc.step = step;
  sa.pc.scale = kOutScale, sa.pc.fB = cam->fx * cam->baseline_mm, sa.pc.fx = cam->fx, sa.pc.fy = cam->fy, sa.pc.cx = cam->cx, sa.pc.cy = cam->cy;
  sa.pc.zmin = cam->z_min_m, sa.pc.zmax = cam->z_max_m;
  bool level = true;
  for (float v : e->p.base_from_cam) level = level && v == 0.f;
  const float level_mount[12] = {0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0};
  memcpy(sa.m, level ? level_mount : e->p.base_from_cam, sizeof sa.m);
  sa.mount_stride = dstride;
  sa.k256f = (float)e->k256, sa.range_max = e->p.range_max_m, sa.zmin_mm = e->zmin_mm, sa.zmax_mm = e->zmax_mm;
  sa.mw = e->p.mw, sa.mh = e->p.mh;
  ElFuseArgs fa{};
  fa.S = e->state, fa.lo_off = (size_t)e->streams * cells;
  fa.mw = e->p.mw, fa.mh = e->p.mh, fa.min_points = e->p.min_points, fa.alpha = e->p.alpha;
  const int cblocks = (Wo + 255) / 256;
  const unsigned slot_chunks = (unsigned)((cells + 255) / 256);
  for (int k0 = 0; k0 < n; k0 += kSlice) {      // the frame lists and the poses of kSlice maps fit the kernel arguments
    const int m = std::min(kSlice, n - k0);
    // a workgroup is 256 columns of a chunk of rows: about 2048 workgroups a launch, and runs of at least 16 rows
    sa.chunks = std::max(1, std::min((2048 + cblocks * m - 1) / (cblocks * m), (Ho + 15) / 16));
    sa.rows = (Ho + sa.chunks - 1) / sa.chunks;
    sa.chunks = (Ho + sa.rows - 1) / sa.rows;
    sa.pc.raw = draw + (size_t)k0 * H * W;
    sa.mounts = dmounts ? dmounts + (size_t)k0 * dstride : nullptr;
    sa.cnt = dcnt + k0 * cells, sa.fmax = dfmax + k0 * cells, sa.fmin = dfmin + k0 * cells;
    memcpy(sa.q, q.data() + (size_t)k0 * 6, (size_t)m * 24);
    const dim3 grid(cblocks * sa.chunks, m);
    if (dmounts) hipLaunchKernelGGL(k_el_scatter<true>, grid, dim3(256), 0, st, sa);
    else hipLaunchKernelGGL(k_el_scatter<false>, grid, dim3(256), 0, st, sa);
    fa.cnt = sa.cnt, fa.fmax = sa.fmax, fa.fmin = sa.fmin;
    fa.hi = dhi + k0 * cells, fa.lo = dlo + k0 * cells;
    fa.stats = dstats ? dstats + (size_t)k0 * 4 : nullptr;
    for (int k = 0; k < m; ++k) fa.org[k][0] = sa.q[k][4], fa.org[k][1] = sa.q[k][5];
    int last[kSlice];      // per group: its last map of the slice
    const int groups = group_slice(fa.g, fa.t, last, stream_of, k0, m, e->fresh.data(), e->ox.data(), e->oy.data());
    hipLaunchKernelGGL(k_el_fuse, dim3(slot_chunks, groups), dim3(256), 0, st, fa);
    HIP_TRY(h, hipGetLastError());
    commit_slice(fa.g, groups, last, sa.q, e->fresh.data(), e->ox.data(), e->oy.data());
  }
  if (dtrav || drise || dstats) {
    ElVerdictArgs va{dhi, dlo, dtrav, drise, dstats, e->p.mw, e->p.mh, e->p.radius, e->p.max_step_mm, (e->p.mw + kElTileW - 1) / kElTileW};
    const int tiles_y = (e->p.mh + kElTileH - 1) / kElTileH;
    hipLaunchKernelGGL(k_el_verdict, dim3(va.tiles_x * tiles_y, n), dim3(256), 0, st, va);
    HIP_TRY(h, hipGetLastError());
  }
  return b.close();
}

// ---- inflation by the robot's radius (csrc/sn_inflate.hpp): a lane of the handle's; the cost table of the last parameter block
// stays on the device, as the obstacle lane keeps its beam edges ------------------------------------------------------------------
int sn_inflate_table(const sn_inflate_params* p, uint8_t* table, int* R) {
  int r = 0;
  if (in_params_check(p, &r)) return SN_ERR_ARG;
  std::vector<uint8_t> T((size_t)r * r + 1);
  if (!in_table(p, r, T.data())) return SN_ERR_ARG;
  if (table) memcpy(table, T.data(), T.size());
  if (R) *R = r;
  return SN_OK;
}

int sn_inflate_grid(sn_handle* h, int n, const int8_t* occ, int gw, int gh, const sn_inflate_params* p, uint8_t* cost, int8_t* grid,
                    uint16_t* dist2, uint32_t* stats, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  auto refuse = [&](const char* why) {
    set_err(h, std::string("sn_inflate_grid: ") + why);
    return SN_ERR_ARG;
  };
  if (!p || !occ) return refuse("a NULL pointer");
  if (n <= 0 || n > h->max_batch) return refuse("n outside 1..max_batch");
  if (gw < 1 || gh < 1 || gw > kInMaxCells || gh > kInMaxCells) return refuse("gw and gh must be 1..4096");
  int R = 0;
  if (const char* why = in_params_check(p, &R)) return refuse(why);
  if (!cost && !grid && !dist2 && !stats) return refuse("one of cost, grid, dist2 and stats is needed");
  if (((uintptr_t)dist2 & 1) || ((uintptr_t)stats & 3)) return refuse("a misaligned buffer");
  const size_t cells = (size_t)gw * gh, map_bytes = n * cells, stats_bytes = (size_t)n * 20;
  {
    const Span in{occ, map_bytes};
    const Span out[4] = {{cost, map_bytes}, {grid, map_bytes}, {dist2, map_bytes * 2}, {stats, stats_bytes}};
    for (int i = 0; i < 4; ++i) {
      if (overlap({in}, {out[i]})) return refuse("overlapping buffers");
      for (int j = i + 1; j < 4; ++j)
        if (overlap({out[i]}, {out[j]})) return refuse("overlapping buffers");
    }
  }
  using I = sn_handle::Inflate;
  I& lane = h->inf;
  Bracket b(h, "sn_inflate_grid", mem, stream, lane);
  Staging& s = b.s;
  hipStream_t st = b.c.st;
  InArgs a{};
  a.occ = s.in(I::kOcc, occ, map_bytes);
  a.cost = s.out(I::kCost, cost, map_bytes);
  a.grid = s.out(I::kGrid, grid, map_bytes);
  a.dist2 = s.out(I::kDist2, dist2, map_bytes * 2);
  a.stats = s.out(I::kStats, stats, stats_bytes);
  uint8_t* dtable = s.scratch<uint8_t>(I::kTable, (size_t)kInMaxR * kInMaxR + 1);
  if (s.rc) return s.rc;
  // The key is tested first, under the lane's lock: a call with the block of the one before builds no table and uploads none.
  // A new block is rare: its table is built here (still nothing launched or written), uploaded behind the lane's earlier calls
  // and waited for.
  if (!lane.cached || memcmp(&lane.key, p, sizeof *p)) {
    std::vector<uint8_t> T((size_t)R * R + 1);
    if (!in_table(p, R, T.data())) return refuse("the cost table increases with the distance");
    lane.cached = false;
    HIP_TRY(h, hipMemcpyAsync(dtable, T.data(), T.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    lane.key = *p, lane.cached = true;
  }
  a.table = dtable;
  a.gw = gw, a.gh = gh, a.R = R, a.lethal_min = p->lethal_min, a.flags = p->flags;
  a.tiles_x = (gw + kInTileW - 1) / kInTileW;
  const unsigned tiles = (unsigned)(a.tiles_x * ((gh + kInTileH - 1) / kInTileH));
  if (a.stats) HIP_TRY(h, hipMemsetAsync(a.stats, 0, stats_bytes, st));
  const bool wide = in_waves((long long)tiles * n, h->num_cu, h->inflate_waves) == 16;
  if (wide) hipLaunchKernelGGL(k_inflate<16>, dim3(tiles, n), dim3(1024), 0, st, a);
  else hipLaunchKernelGGL(k_inflate<4>, dim3(tiles, n), dim3(256), 0, st, a);
  HIP_TRY(h, hipGetLastError());
  return b.close();
}

// ---- navigation function and path (csrc/sn_navfn.hpp): a lane of the handle's.  The rounds of the relaxation are separate
// launches; max_rounds == 0 reads the work word back every kNavChunk of them ----------------------------------------------------
int sn_navfn(sn_handle* h, int n, const uint8_t* cost, int gw, int gh, const int32_t* goals, const int32_t* starts, const sn_nav_params* p,
             uint32_t* potential, int32_t* path, uint32_t* stats, int* rounds_out, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  auto refuse = [&](const char* why) {
    set_err(h, std::string("sn_navfn: ") + why);
    return SN_ERR_ARG;
  };
  if (!p || !cost || !goals) return refuse("a NULL pointer");
  if (n <= 0 || n > h->max_batch) return refuse("n outside 1..max_batch");
  if (gw < 1 || gh < 1 || gw > kNavMaxSide || gh > kNavMaxSide) return refuse("gw and gh must be 1..4096");
  if ((long long)gw * gh > SN_NAV_MAX_CELLS) return refuse("gw * gh must be at most 2^20");
  if (const char* why = nav_params_check(p)) return refuse(why);
  if (!potential && !path && !stats) return refuse("one of potential, path and stats is needed");
  if (path && (!starts || p->max_path == 0)) return refuse("path needs starts and max_path > 0");
  if (((uintptr_t)goals | (uintptr_t)starts | (uintptr_t)potential | (uintptr_t)path | (uintptr_t)stats) & 3) return refuse("a misaligned buffer");
  const size_t cells = (size_t)gw * gh, cost_bytes = n * cells, pot_bytes = cost_bytes * 4, cell_bytes = (size_t)n * 8,
               path_bytes = (size_t)n * p->max_path * 8, stats_bytes = (size_t)n * 20;
  {
    const Span all[6] = {{cost, cost_bytes}, {goals, cell_bytes}, {starts, cell_bytes}, {potential, pot_bytes}, {path, path_bytes},
                         {stats, stats_bytes}};
    for (int i = 0; i < 6; ++i)
      for (int j = i + 1; j < 6; ++j)
        if (overlap({all[i]}, {all[j]})) return refuse("overlapping buffers");
  }
  using N = sn_handle::Nav;
  N& lane = h->nav;
  Bracket b(h, "sn_navfn", mem, stream, lane);
  Staging& s = b.s;
  hipStream_t st = b.c.st;
  const bool converge = p->max_rounds == 0;
  if (converge) b.c.blocking = true;      // the host reads the work word between the chunks anyway
  NavArgs a{};
  a.gw = gw, a.gh = gh, a.maps = n;
  a.tiles_x = (gw + kNavTW - 1) / kNavTW, a.tiles_y = (gh + kNavTH - 1) / kNavTH;
  a.neutral = p->neutral, a.lethal = p->lethal_cost, a.unknown_cost = p->unknown_cost, a.flags = p->flags, a.max_path = p->max_path;
  const size_t tiles = (size_t)a.tiles_x * a.tiles_y, marks_bytes = (1 + 2 * (size_t)n * tiles) * 4;
  a.cost = s.in(N::kCost, cost, cost_bytes);
  a.goals = s.in(N::kGoals, goals, cell_bytes);
  a.starts = starts ? s.in(N::kStarts, starts, cell_bytes) : nullptr;
  a.pot = s.out(N::kPot, potential, pot_bytes, true);
  a.path = s.inout(N::kPath, path, path_bytes);      // entries past the path's length keep the caller's bytes
  a.stats = s.out(N::kStats, stats, stats_bytes);
  a.work = s.scratch<uint32_t>(N::kMarks, marks_bytes);
  uint32_t* pin = s.scratch<uint32_t>(N::kPinWork, 4);
  if (s.rc) return s.rc;
  a.marks = a.work + 1;
  HIP_TRY(h, hipMemsetAsync(a.work, 0, marks_bytes, st));
  if (a.stats) HIP_TRY(h, hipMemsetAsync(a.stats, 0, stats_bytes, st));
  const dim3 per_cell((unsigned)((cells + 255) / 256), n);
  hipLaunchKernelGGL(k_nav_init, per_cell, dim3(256), 0, st, a);
  int rounds = 0;
  if (converge) {
    // at most 1 + gw * gh rounds do work, so the loop ends; the cap only names a broken device
    for (bool left = true; left;) {
      for (int i = 0; i < kNavChunk; ++i) hipLaunchKernelGGL(k_nav_relax, dim3((unsigned)tiles, n), dim3(kNavThreads), 0, st, a, rounds++);
      HIP_TRY(h, hipGetLastError());
      HIP_TRY(h, hipMemcpyAsync(pin, a.work, 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(h, hipStreamSynchronize(st));
      left = (long long)*pin >= rounds;      // the chunk's last round was active
      if (left && (size_t)rounds > cells + 1 + kNavChunk) {
        set_err(h, "sn_navfn: the relaxation did not converge within 1 + gw * gh rounds");
        return SN_ERR_DEVICE;
      }
    }
  } else {
    for (; rounds < p->max_rounds; ++rounds) hipLaunchKernelGGL(k_nav_relax, dim3((unsigned)tiles, n), dim3(kNavThreads), 0, st, a, rounds);
  }
  if (a.stats) hipLaunchKernelGGL(k_nav_stats, per_cell, dim3(256), 0, st, a, rounds, converge ? 0 : 1);
  if (a.starts && (a.path || a.stats)) hipLaunchKernelGGL(k_nav_path, dim3(n), dim3(64), 0, st, a);
  HIP_TRY(h, hipGetLastError());
  if (!converge && b.c.blocking) HIP_TRY(h, hipMemcpyAsync(pin, a.work, 4, hipMemcpyDeviceToHost, st));
  if (int rc = b.close()) return rc;
  if (rounds_out) *rounds_out = b.c.blocking ? (int)*pin : -1;
  return SN_OK;
}

// ---- trajectory rollout (csrc/sn_rollout.hpp): a lane of the handle's; the tables of the last (parameters, footprint) pair stay
// on the device, as the inflation lane keeps its cost table -----------------------------------------------------------------------
int sn_rollout_tables(const sn_rollout_params* p, const float* footprint, int nf, int32_t* centres, int32_t* offsets) {
  if (ro_params_check(p, footprint, nf)) return SN_ERR_ARG;
  return ro_tables(p, footprint, nf, centres, offsets) ? SN_ERR_ARG : SN_OK;
}

int sn_rollout_pose_q(float cell_m, double origin_x_m, double origin_y_m, const double* pose, int32_t* q) {
  if (!pose || !q) return SN_ERR_ARG;
  int32_t tmp[5];
  if (!ro_pose_q(cell_m, origin_x_m, origin_y_m, pose, tmp)) return SN_ERR_ARG;
  memcpy(q, tmp, sizeof tmp);
  return SN_OK;
}

int sn_rollout_velocity(const sn_rollout_params* p, int s, double* out) {
  if (!out || ro_params_check(p, nullptr, 0) || s < 0 || s >= p->nv * p->nw) return SN_ERR_ARG;
  out[0] = ro_lattice(p->v_min, p->v_max, p->nv, s / p->nw);
  out[1] = ro_lattice(p->w_min, p->w_max, p->nw, s % p->nw);
  return SN_OK;
}

int sn_rollout(sn_handle* h, int n, const uint8_t* cost, const uint32_t* potential, int gw, int gh, const int32_t* poses_q,
               const int32_t* window, const sn_rollout_params* p, const float* footprint, int nf, uint32_t* samples, uint32_t* best,
               int32_t* traj, int mem, void* stream) {
  if (!h) return SN_ERR_ARG;
  auto refuse = [&](const char* why) {
    set_err(h, std::string("sn_rollout: ") + why);
    return SN_ERR_ARG;
  };
  if (!p || !cost || !potential || !poses_q) return refuse("a NULL pointer");
  if (n <= 0 || n > h->max_batch) return refuse("n outside 1..max_batch");
  if (gw < 1 || gh < 1 || gw > kRoMaxSide || gh > kRoMaxSide) return refuse("gw and gh must be 1..4096");
  if ((long long)gw * gh > SN_NAV_MAX_CELLS) return refuse("gw * gh must be at most 2^20");
  if (const char* why = ro_params_check(p, footprint, nf)) return refuse(why);
  if (!samples && !best && !traj) return refuse("one of samples, best and traj is needed");
  if (((uintptr_t)potential | (uintptr_t)poses_q | (uintptr_t)window | (uintptr_t)samples | (uintptr_t)best | (uintptr_t)traj) & 3)
    return refuse("a misaligned buffer");
  const int S = p->nv * p->nw, steps1 = p->steps + 1;
  const size_t cells = (size_t)gw * gh, cost_bytes = n * cells, pot_bytes = cost_bytes * 4, pose_bytes = (size_t)n * 20,
               win_bytes = (size_t)n * 16, samples_bytes = (size_t)n * S * 8, best_bytes = (size_t)n * 32,
               traj_bytes = (size_t)n * steps1 * 12;
  {
    const Span all[7] = {{cost, cost_bytes}, {potential, pot_bytes}, {poses_q, pose_bytes}, {window, win_bytes},
                         {samples, samples_bytes}, {best, best_bytes}, {traj, traj_bytes}};
    for (int i = 0; i < 7; ++i)
      for (int j = i + 1; j < 7; ++j)
        if (overlap({all[i]}, {all[j]})) return refuse("overlapping buffers");
  }
  using R = sn_handle::Rollout;
  R& lane = h->roll;
  const size_t centres_bytes = (size_t)S * steps1 * 12, offsets_bytes = (size_t)p->nw * steps1 * nf * 8;
  auto cached = [&] {      // under the lane's lock: the device holds the tables of this (parameters, footprint) pair
    return lane.cached && lane.key_nf == nf && !memcmp(&lane.key, p, sizeof *p) && (nf == 0 || !memcmp(lane.key_fp, footprint, (size_t)nf * 8));
  };
  // The key is tested first: a call with the pair of the one before builds no tables and uploads none.  A new pair is rare: its
  // tables are built here, before the call is opened on any stream, so that a pair whose arcs reach too far is refused like
  // every other bad argument; they are uploaded below, behind the lane's earlier calls, and waited for.
  std::vector<int32_t> hc, ho;
  auto build = [&]() -> const char* {
    hc.resize(centres_bytes / 4), ho.resize(offsets_bytes / 4);
    return ro_tables(p, footprint, nf, hc.data(), ho.data());
  };
  {
    std::lock_guard<std::mutex> lk(lane.mu);
    if (!cached())
      if (const char* why = build()) return refuse(why);
  }
  Bracket b(h, "sn_rollout", mem, stream, lane);
  Staging& s = b.s;
  hipStream_t st = b.c.st;
  if (s.rc) return s.rc;
  const bool hit = cached();
  if (!hit && hc.empty()) build();      // another thread's pair came in between; this one was accepted when it was cached
  RoArgs a{};
  int32_t* dcentres = s.scratch<int32_t>(R::kCentres, centres_bytes);
  int32_t* doffsets = s.scratch<int32_t>(R::kOffsets, offsets_bytes ? offsets_bytes : 8);
  if (s.rc) return s.rc;
  if (!hit) {
    lane.cached = false;
    HIP_TRY(h, hipMemcpyAsync(dcentres, hc.data(), centres_bytes, hipMemcpyHostToDevice, st));
    if (offsets_bytes) HIP_TRY(h, hipMemcpyAsync(doffsets, ho.data(), offsets_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    lane.key = *p, lane.key_nf = nf, lane.cached = true;
    if (nf) memcpy(lane.key_fp, footprint, (size_t)nf * 8);
  }
  a.cost = s.in(R::kCost, cost, cost_bytes);
  a.pot = s.in(R::kPot, potential, pot_bytes);
  a.poses = s.in(R::kPoses, poses_q, pose_bytes);
  a.window = window ? s.in(R::kWindow, window, win_bytes) : nullptr;
  a.samples = s.out(R::kSamples, samples, samples_bytes, true);
  a.best = s.out(R::kBest, best, best_bytes);
  a.traj = s.inout(R::kTraj, traj, traj_bytes);      // a map without a valid sample keeps the caller's bytes
  if (s.rc) return s.rc;
  a.centres = dcentres, a.offsets = doffsets;
  a.gw = gw, a.gh = gh, a.nv = p->nv, a.nw = p->nw, a.T = p->steps, a.nf = nf;
  a.lethal = p->lethal_cost, a.centre_lethal = p->centre_lethal_cost, a.unknown_cost = p->unknown_cost, a.flags = p->flags;
  a.w_goal = p->w_goal, a.w_occ = p->w_occ;
  const unsigned groups = (unsigned)(p->nw * ((p->nv + kRoWaves - 1) / kRoWaves));
  const size_t lds = std::max<size_t>((size_t)steps1 * nf * 8, 8);
  hipLaunchKernelGGL(k_rollout_eval, dim3(groups, n), dim3(kRoThreads), lds, st, a);
  if (a.best || a.traj) hipLaunchKernelGGL(k_rollout_best, dim3(n), dim3(kRoBestThreads), 0, st, a);
  HIP_TRY(h, hipGetLastError());
  return b.close();
}

}  // extern "C"
