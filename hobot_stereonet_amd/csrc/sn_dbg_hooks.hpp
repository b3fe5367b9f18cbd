// sn_dbg_hooks.hpp — the sn_dbg_* entry points (parity hooks: one kernel or block on caller-supplied tensors, as the
// pipeline launches it) and the host-side marshalling they share: split-slot tensors, their zero-bordered grids
// (PaddedSlots), the fp16 tower layout (RefHost), its device allocation with front rows and slack (RefDev) and the sequence
// the tower hooks run around their launch line (TowerHook), the guarded
// outputs of the mid-stage hooks (Guarded, HookStat), and the grid cap of the hooks (sn_dbg_set_grid_cus, dbg_cus).  Part of
// the single translation unit stereonet_hip.hip.
#pragma once

namespace {

// host <-> split-slot layout (SlotIn): src/dst fp32 [nimg][32][H][W]
void host_to_slots(const float* src, int nimg, int H, int W, std::vector<_Float16>& dst) {
  const size_t plane = (size_t)H * W;
  dst.assign((size_t)nimg * 8 * plane * 8, (_Float16)0.f);
  for (int img = 0; img < nimg; ++img)
    for (int c = 0; c < kC; ++c)
      for (size_t i = 0; i < plane; ++i) {
        const float v = src[((size_t)img * kC + c) * plane + i];
        const _Float16 hi = (_Float16)v;
        const size_t base = (((size_t)img * 4 + (c >> 3)) * 2) * plane;
        dst[(base + i) * 8 + (c & 7)] = hi;
        dst[(base + plane + i) * 8 + (c & 7)] = (_Float16)((v - (float)hi) * kSplitScale);
      }
}
void host_from_slots(const std::vector<_Float16>& src, int nimg, int H, int W, float* dst) {
  const size_t plane = (size_t)H * W;
  for (int img = 0; img < nimg; ++img)
    for (int c = 0; c < kC; ++c)
      for (size_t i = 0; i < plane; ++i) {
        const size_t base = (((size_t)img * 4 + (c >> 3)) * 2) * plane;
        dst[((size_t)img * kC + c) * plane + i] =
            (float)src[(base + i) * 8 + (c & 7)] + (float)src[(base + plane + i) * 8 + (c & 7)] * kSplitInv;
      }
}

template <class V>
hipError_t to_dev(void* dev, const V& v) {
  return hipMemcpy(dev, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice);
}
template <class V>
hipError_t from_dev(V& v, const void* dev) {
  return hipMemcpy(v.data(), dev, v.size() * sizeof(v[0]), hipMemcpyDeviceToHost);
}

// Host image of split-slot (block, part) planes inside a zero-bordered grid (FeatPad, SlotGeom, VolPad): `nplanes` planes
// of g.PH x g.PW slots with the H x W image at (g.py, g.px), and `lead` all-zero planes in front of and behind them
// (VolPad: one disparity plane = 8).  group > 0: the planes come in groups of `group` (VolPad: the 8 Dl planes of one pair)
// with `lead` zero planes in front of the first group and behind EVERY group, so two neighbours share one run of zero
// planes.  The plain counterpart is [nplanes][H][W] slots (host_to_slots).
struct PaddedSlots {
  SlotGeom g;
  int H, W;
  size_t nplanes, lead, group;
  std::vector<_Float16> v;
  PaddedSlots(const SlotGeom& g_, int H_, int W_, size_t nplanes_, size_t lead_ = 0, size_t group_ = 0)
      : g(g_), H(H_), W(W_), nplanes(nplanes_), lead(lead_), group(group_ ? group_ : (nplanes_ ? nplanes_ : 1)),
        v((lead_ + (nplanes_ + group - 1) / group * (group + lead_)) * g_.PH * g_.PW * 8, (_Float16)0.f) {}
  size_t padded_plane(size_t plane) const { return lead + plane / group * (group + lead) + plane % group; }
  size_t row(size_t plane, int y) const { return ((padded_plane(plane) * g.PH + y + g.py) * g.PW + g.px) * 8; }
  void put(const std::vector<_Float16>& plain) {
    for (size_t p = 0; p < nplanes; ++p)
      for (int y = 0; y < H; ++y) memcpy(&v[row(p, y)], &plain[((p * H + y) * W) * 8], (size_t)W * 16);
  }
  void get(std::vector<_Float16>& plain) const {
    for (size_t p = 0; p < nplanes; ++p)
      for (int y = 0; y < H; ++y) memcpy(&plain[((p * H + y) * W) * 8], &v[row(p, y)], (size_t)W * 16);
  }
  bool outside_is_zero() const {
    const size_t phw = (size_t)g.PH * g.PW;
    for (size_t i = 0; i < v.size(); ++i) {
      const size_t sl = i / 8, p = sl / phw, y = (sl % phw) / g.PW, x = sl % g.PW;
      const bool inside = p >= lead && (p - lead) % (group + lead) < group && y >= (size_t)g.py && y < (size_t)H + g.py &&
                          x >= (size_t)g.px && x < (size_t)W + g.px;
      if (!inside && (float)v[i] != 0.f) return false;
    }
    return true;
  }
};

// Host image of the fp16 tower tensors: n images of 32 x h x w as NCHW8c inside the zero border of RefGeom g.  split: the
// layout holds a lo tensor lo_slots behind the hi tensor; slack: each part is followed by ref_slack(g) slots.
struct RefHost {
  RefGeom g{};
  int n = 0, h = 0, w = 0;
  size_t lo_slots = 0;
  std::vector<_Float16> v;
  RefHost() = default;
  RefHost(const RefGeom& g_, int n_, int h_, int w_, bool split, bool slack)
      : g(g_), n(n_), h(h_), w(w_), lo_slots(ref16_slots(g_, n_) + (slack ? ref_slack(g_) : 0)), v((split ? 2 : 1) * lo_slots * 8) {}
  size_t slots() const { return v.size() / 8; }
  size_t at(int i, int c, int y, int x) const {
    return ((((size_t)i * 4 + (c >> 3)) * g.Hs + y + kRefPad) * g.Ws + x + kRefPad) * 8 + (c & 7);
  }
  void pack(const float* src, bool split) {      // src fp32 [n][32][h][w]
    v.assign(v.size(), (_Float16)0.f);
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < kC; ++c)
        for (int y = 0; y < h; ++y)
          for (int x = 0; x < w; ++x) {
            const float f = src[(((size_t)i * kC + c) * h + y) * w + x];
            const _Float16 hi = (_Float16)f;
            v[at(i, c, y, x)] = hi;
            if (split) v[lo_slots * 8 + at(i, c, y, x)] = (_Float16)((f - (float)hi) * kSplitScale);
          }
  }
  void unpack(float* dst, bool split) const {
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < kC; ++c)
        for (int y = 0; y < h; ++y)
          for (int x = 0; x < w; ++x) {
            float f = (float)v[at(i, c, y, x)];
            if (split) f += (float)v[lo_slots * 8 + at(i, c, y, x)] * kSplitInv;
            dst[(((size_t)i * kC + c) * h + y) * w + x] = f;
          }
  }
  // the 0xff pattern (fp16 NaN) in the valid area of the first `parts` tensors, zeros everywhere else: what an output
  // tensor holds before the launch, so that an element the kernel does not write shows
  void prefill(int parts) {
    v.assign(v.size(), (_Float16)0.f);
    for (int part = 0; part < parts; ++part)
      for (int plane = 0; plane < 4 * n; ++plane)
        for (int y = 0; y < h; ++y)
          memset(&v[part * lo_slots * 8 + (((size_t)plane * g.Hs + y + kRefPad) * g.Ws + kRefPad) * 8], 0xff, (size_t)w * 16);
  }
  // everything but the valid area of the first `parts` tensors is still zero after a kernel: the border of all n images,
  // the slack behind each part, and a lo part the kernel was not asked to write
  bool outside_is_zero(int parts) const {
    const size_t tensor = ref16_slots(g, n), hw = (size_t)g.Hs * g.Ws;
    for (size_t s = 0; s < slots(); ++s) {
      const size_t part = s / lo_slots, t = s % lo_slots, y = t % hw / g.Ws, x = t % g.Ws;
      if ((int)part < parts && t < tensor && y >= (size_t)kRefPad && y < (size_t)kRefPad + h && x >= (size_t)kRefPad &&
          x < (size_t)kRefPad + w)
        continue;
      for (int e = 0; e < 8; ++e)
        if ((float)v[s * 8 + e] != 0.f) return false;
    }
    return true;
  }
};

// a zeroed fp16 tower tensor behind its front rows (alloc_ref16), owned by ds
hipError_t alloc_ref16(DevScope& ds, const RefGeom& g, size_t tensor_and_slack_slots, uint4** base) {
  uint4* raw = nullptr;
  const hipError_t e = alloc_ref16(g, tensor_and_slack_slots, &raw, base);
  ds.track(raw);
  return e;
}

// A device fp16 tower tensor as the pipeline allocates it, [front | tensor | slack] (alloc_ref16), owned by ds; t is its host
// image (built with slack).
struct RefDev {
  uint4* base = nullptr;      // the tensor: what the kernels are handed
  size_t front = 0;
  hipError_t alloc(DevScope& ds, const RefHost& t) {
    front = ref_front(t.g);
    return alloc_ref16(ds, t.g, t.slots(), &base);
  }
  // reads the tensor into t; *ok: the front rows, the border of every image and the slack still hold their zeros
  hipError_t get(RefHost& t, int parts, bool* ok) const {
    std::vector<_Float16> f(front * 8);
    hipError_t e = from_dev(f, base - front);
    if (e == hipSuccess) e = from_dev(t.v, base);
    *ok = e == hipSuccess && t.outside_is_zero(parts);
    for (const _Float16 x : f) *ok = *ok && (float)x == 0.f;
    return e;
  }
};
#define SN_REF_GET(h, dev, t, parts, what)                                                     \
  do {                                                                                         \
    bool ok_ = false;                                                                          \
    HIP_TRY(h, (dev).get(t, parts, &ok_));                                                     \
    if (!ok_) {                                                                                \
      set_err(h, std::string(what) + " wrote outside the valid area (border, front rows or slack)"); \
      return SN_ERR_DEVICE;                                                                    \
    }                                                                                          \
  } while (0)

// The CU count a parity hook sizes its grid with: sn_dbg_set_grid_cus, or the device's.  banded: the launcher builds its grid
// in XCD bands of 8, so a cap that is no multiple of 8 is refused (launch_down01 would launch nothing).
int dbg_cus(const sn_handle* h) { return h->dbg_grid_cus > 0 ? h->dbg_grid_cus : h->num_cu; }
#define SN_DBG_BANDED(h)                                                            \
  do {                                                                              \
    if (h->dbg_grid_cus % 8) {                                                      \
      set_err(h, "this hook's launcher builds its grid in bands of 8: sn_dbg_set_grid_cus needs a multiple of 8"); \
      return SN_ERR_ARG;                                                            \
    }                                                                               \
  } while (0)

// What every tower hook does around its launch line.  begin(): the argument checks, the device, the geometry, the layers, the
// two tensors as the pipeline allocates them and what they hold before the launch.  run(): the launch between a device
// synchronisation (the uploads are hipMemcpy on the null stream, the launch goes onto h->stream) and the stream's, then the
// read-back of EVERY tensor (front rows, border of all n images, slack) and the result.
enum : unsigned {
  kTowerSplit = 1,      // hi / lo operands (SN_PREC_F16X3): tensors [hi | slack | lo | slack], layers through upload_ref_f16x3
  kTowerHiOnly = 2,     // (with kTowerSplit) the kernel writes the hi part alone: the lo part has to stay zero
  kTowerBanded = 4,     // the launcher builds its grid in XCD bands (SN_DBG_BANDED)
  kTowerQueue = 8,      // the launcher hands out tiles from ws.tile_ctr, which only an engine created in an fp16 mode has
};
struct TowerHook {
  struct WB { const float *w, *b; };      // one 32 -> 32 3x3 layer: w [32][32][3][3], b [32]
  sn_handle* const h;
  const std::string what, what_other;     // whose fault a changed border is: of the result tensor, of the other one
  DevScope ds;          // frees every tracked device buffer on every return path
  RefHost t;            // the host image both tensors are filled from and read into
  RefLayerF16 L[2];
  RefDev x, y;          // x: the input (none when the hook has no tower tensor to read), y: the other tensor
  uint4* res = nullptr; // the tensor that holds the result after the launch: y, unless the launch line says x
  int parts = 1;
  TowerHook(sn_handle* h_, const std::string& what_) : h(h_), what(what_), what_other(what_ + " (its other tensor)") {}
  TowerHook(sn_handle* h_, const std::string& what_, const std::string& other) : h(h_), what(what_), what_other(other) {}

  // need: the caller's pointers, none of which may be null.  in (nullable): fp32 [n][32][hgt][wid], packed into x.  residual
  // (nullable): packed into y, the in-place form of the pipeline; without one y starts as the 0xff pattern, as every output
  // that is not also an input.
  int begin(std::initializer_list<const void*> need, int n, int hgt, int wid, int dil, unsigned flags, const float* in,
            const float* residual, std::initializer_list<WB> layers) {
    if (!h || n <= 0 || hgt <= 0 || wid <= 0 || (dil != 1 && dil != 2 && dil != 4 && dil != 8)) return SN_ERR_ARG;
    for (const void* p : need)
      if (!p) return SN_ERR_ARG;
    if (flags & kTowerBanded) SN_DBG_BANDED(h);
    int rc = check_device(h);
    if (rc) return rc;
    if ((flags & kTowerQueue) && !h->ws.tile_ctr) {
      set_err(h, what + ": this hook needs an engine created in an fp16 mode");
      return SN_ERR_ARG;
    }
    const RefGeom g = make_ref_geom(hgt, wid);
    // the tower kernels add 32-bit byte offsets to a tensor's base (sn_create refuses such a workspace)
    if ((ref16_slots(g, n) + ref_slack(g) + ref_front(g)) * 16 >= ((size_t)1 << 32)) return SN_ERR_ARG;
    const bool split = (flags & kTowerSplit) != 0;
    parts = split && !(flags & kTowerHiOnly) ? 2 : 1;
    t = RefHost(g, n, hgt, wid, split, true);
    RefLayerF16* l = L;
    for (const WB& wb : layers) {
      const HostLayer hl{wb.w, wb.b, kC, kC, 9};
      if (!rc) rc = split ? upload_ref_f16x3(h, hl, l) : upload_ref_f16(h, hl, switches_at_create().w_round_sum_preserving, l);
      ds.adopt(*l++);
    }
    if (rc) return rc;
    if (in) {
      HIP_TRY(h, x.alloc(ds, t));
      t.pack(in, parts == 2);
      HIP_TRY(h, to_dev(x.base, t.v));
    }
    HIP_TRY(h, y.alloc(ds, t));
    if (residual) t.pack(residual, parts == 2);
    else t.prefill(parts);
    HIP_TRY(h, to_dev(y.base, t.v));
    res = y.base;
    if (flags & kTowerQueue) HIP_TRY(h, hipMemsetAsync(h->ws.tile_ctr, 0, kTileCtrBytes, h->stream));
    return SN_OK;
  }

  // launch: () -> hipError_t, the hook's launch line(s).  out (nullable): fp32 [n][32][hgt][wid], the result tensor.
  template <class Launch>
  int run(float* out, Launch launch) {
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, launch());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const bool in_x = x.base && res == x.base;
    if (x.base) SN_REF_GET(h, in_x ? y : x, t, parts, what_other);
    SN_REF_GET(h, in_x ? x : y, t, parts, what);
    if (out) t.unpack(out, parts == 2);
    return SN_OK;
  }
};

// A device output of a mid-stage hook between two guard bands of kGuardBytes known bytes (kGuardByte), owned by ds.  The
// payload starts as the 0xff pattern (fp32 NaN, int32 -1, fp16 NaN): an element the kernel does not write shows.
constexpr size_t kGuardBytes = 4096;
constexpr int kGuardByte = 0xa5;
template <class T>
struct Guarded {
  char* raw = nullptr;
  size_t bytes = 0;
  T* p() const { return reinterpret_cast<T*>(raw + kGuardBytes); }
  hipError_t alloc(DevScope& ds, size_t count) {
    bytes = (count * sizeof(T) + 15) / 16 * 16;
    hipError_t e = ds.alloc(&raw, bytes + 2 * kGuardBytes);
    if (e == hipSuccess) e = hipMemset(raw, kGuardByte, bytes + 2 * kGuardBytes);
    if (e == hipSuccess) e = memset_now(raw + kGuardBytes, 0xff, bytes);
    return e;
  }
  // *ok: both bands still hold kGuardByte
  hipError_t intact(bool* ok) const {
    std::vector<unsigned char> band(2 * kGuardBytes);
    hipError_t e = hipMemcpy(band.data(), raw, kGuardBytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(band.data() + kGuardBytes, raw + kGuardBytes + bytes, kGuardBytes, hipMemcpyDeviceToHost);
    *ok = e == hipSuccess;
    for (unsigned char b : band) *ok = *ok && b == (unsigned char)kGuardByte;
    return e;
  }
};
#define SN_GUARD_CHECK(h, buf, what)                                                \
  do {                                                                              \
    bool ok_ = false;                                                               \
    HIP_TRY(h, (buf).intact(&ok_));                                                 \
    if (!ok_) {                                                                     \
      set_err(h, std::string(what) + " wrote outside its output (guard band)");     \
      return SN_ERR_DEVICE;                                                         \
    }                                                                               \
  } while (0)

// One statistic word of a hook's own (the layout refine_stat_commit / lowres_nonfinite_commit write): zeroed, owned by ds
struct HookStat {
  unsigned long long* dev = nullptr;
  hipError_t alloc(DevScope& ds) {
    const hipError_t e = ds.alloc(&dev, (size_t)kStatWordStride);
    return e != hipSuccess ? e : memset_now(dev, 0, kStatWordStride * sizeof(unsigned long long));
  }
  // the sum over the slots of the 64-bit word `at` of every line (0 = the |D r| sum, kStatNonfinite, kStatNonfiniteLow)
  hipError_t read(int at, unsigned long long* out) const {
    std::vector<unsigned long long> v(kStatWordStride);
    const hipError_t e = from_dev(v, dev);
    *out = 0;
    for (int s = 0; s < kStatSlots; ++s) *out += v[(size_t)s * kStatLine + at];
    return e;
  }
};

// caller volume [n][32][Dl][hl][wl] (PyTorch) -> device order [n Dl][32][hl][wl]
void vol_to_device_order(const float* in, int n, int Dl, size_t plane, std::vector<float>& out) {
  out.resize((size_t)n * Dl * kC * plane);
  for (int i = 0; i < n; ++i)
    for (int ci = 0; ci < kC; ++ci)
      for (int z = 0; z < Dl; ++z)
        memcpy(&out[(((size_t)i * Dl + z) * kC + ci) * plane], &in[(((size_t)i * kC + ci) * Dl + z) * plane], plane * 4);
}

// the padded volume image (VolPad) of n pairs of Dl planes: 8 (block, part) planes per disparity plane, one zero disparity
// plane in front of every pair's planes and one behind the last
PaddedSlots vol_padded(const VolPad& g, int n) {
  return PaddedSlots(SlotGeom{g.PH, g.PW, 1, 1}, g.H, g.W, (size_t)n * g.Dl * 8, 8, (size_t)g.Dl * 8);
}

}  // namespace

extern "C" {

// ---- parity hooks ----------------------------------------------------------------------------------------
int sn_dbg_set_grid_cus(sn_handle* h, int cus) {
  if (!h || cus < 0 || cus > h->num_cu) return SN_ERR_ARG;
  h->dbg_grid_cus = cus;
  return SN_OK;
}

int sn_dbg_last_launch(sn_handle* h, int* wgs, int* units) {
  if (!h || !wgs || !units) return SN_ERR_ARG;
  *wgs = h->dbg_launch.wgs;
  *units = h->dbg_launch.units;
  return SN_OK;
}

// What the async slots did over the handle's life (submit_common): *enabled = hipGraph replay is still on (0: SN_NO_GRAPH, or
// a capture failed and the slots fell back to plain launches), *instantiated = graphs instantiated, *launches = requests
// served by hipGraphLaunch.  Tests only: not declared in include/stereonet_hip.h.
int sn_dbg_slot_graphs(sn_handle* h, int* enabled, int* instantiated, int* launches) {
  if (!h || !enabled || !instantiated || !launches) return SN_ERR_ARG;
  std::lock_guard<std::mutex> lk(h->mu);
  *enabled = h->use_graphs ? 1 : 0;
  *instantiated = h->graphs_instantiated;
  *launches = h->graph_launches;
  return SN_OK;
}

int sn_dbg_conv2d_n(sn_handle* h, int n, const float* in, int cin, int h_px, int w, const float* wt, const float* bias,
                    int k, int stride, int dil, int lrelu, int form, const float* residual, float* out) {
  DevScope ds;      // frees every tracked device buffer on every return path
  if (!h || !in || !wt || !bias || !out || cin <= 0 || cin > kC || n <= 0) return SN_ERR_ARG;
  if (!((k == 3 && stride == 1) || (k == 5 && stride == 2 && dil == 1))) return SN_ERR_ARG;
  int rc = check_device(h);
  if (rc) return rc;
  const int taps = k * k;
  const int Ho = stride == 1 ? h_px : h_px / 2, Wo = stride == 1 ? w : w / 2;
  if (stride == 2 && ((h_px & 1) || (w & 1))) return SN_ERR_ARG;
  if (form < SN_DBG_CONV_F32 || form > SN_DBG_CONV_SLOTS_DMA) return SN_ERR_ARG;
  const bool dma = form == SN_DBG_CONV_SLOTS_DMA, slots = dma || form == SN_DBG_CONV_SLOTS, tower32 = form == SN_DBG_CONV_TOWER32;
  if (slots && !(cin == kC && dil == 1)) return SN_ERR_ARG;     // the split-operand kernels
  if (dma && k == 5 && residual) return SN_ERR_ARG;             // k_down_x3s_dma adds none
  if (slots) SN_DBG_BANDED(h);
  const int ncu = dbg_cus(h);
  LaunchInfo* const li = &h->dbg_launch;
  *li = LaunchInfo{};
  ConvLayer L;
  rc = upload_conv2d(h, HostLayer{wt, bias, kC, cin, taps}, slots ? 8 : (k == 5 || cin <= 4) ? 4 : 8, &L);
  if (!rc && slots)
    rc = upload_x3(h, kC, [&](int co, int c, int tap) { return wt[((size_t)co * kC + c) * taps + tap]; }, &L, taps);
  ds.adopt(L);
  if (rc) return rc;
  hipStream_t st = h->stream;
  if (slots) {          // split-slot tensors in and out through the weights-stationary kernel (fp16 modes' low-res path)
    std::vector<_Float16> hin, hres, hout((size_t)n * 8 * Ho * Wo * 8);
    host_to_slots(in, n, h_px, w, hin);
    if (residual) host_to_slots(residual, n, Ho, Wo, hres);
    else memset(hout.data(), 0xff, hout.size() * 2);      // an output that is not also an input starts as the 0xff pattern
    if (dma) {      // zero-bordered tensors: k_feat_x3s_dma (3x3; input, output and residual in FeatPad) or k_down_x3s_dma
      const FeatPad fp = feat_pad(h_px, w);
      // (5x5 stride 2: an output grid with a border of its own, 3 pixels of slack)
      PaddedSlots pin(k == 3 ? SlotGeom{fp.PH, fp.PW, 1, 1} : down_in_geom(Ho, Wo), h_px, w, (size_t)n * 8);
      PaddedSlots pout(k == 3 ? pin.g : SlotGeom{Ho + 5, Wo + 7, 2, 3}, Ho, Wo, (size_t)n * 8);
      pin.put(hin);
      pout.put(residual ? hres : hout);
      uint4 *pdin = nullptr, *pdout = nullptr;
      HIP_TRY(h, ds.alloc(&pdin, pin.v.size() / 8));
      HIP_TRY(h, ds.alloc(&pdout, pout.v.size() / 8));
      HIP_TRY(h, to_dev(pdin, pin.v));
      HIP_TRY(h, to_dev(pdout, pout.v));
      HIP_TRY(h, hipDeviceSynchronize());
      if (k == 5)
        HIP_TRY(h, launch_down_dma(st, L, pdin, n, Ho, Wo, pdout, pout.g, lrelu != 0, ncu, li));
      else if (residual)
        HIP_TRY(h, (launch_feat_dma<true, true>(st, L, pdin, fp, n, pdout, pdout, lrelu != 0, ncu, li)));     // in place, as the pipeline
      else
        HIP_TRY(h, (launch_feat_dma<true, false>(st, L, pdin, fp, n, pdout, nullptr, lrelu != 0, ncu, li)));
      HIP_TRY(h, hipStreamSynchronize(st));
      HIP_TRY(h, from_dev(pout.v, pdout));
      pout.get(hout);
      if (!pout.outside_is_zero()) {
        set_err(h, k == 3 ? "k_feat_x3s_dma wrote outside the image" : "k_down_x3s_dma wrote outside the image");
        return SN_ERR_DEVICE;
      }
    } else {
      uint4* din = nullptr;
      Guarded<uint4> dout;
      HIP_TRY(h, ds.alloc(&din, hin.size() / 8));
      HIP_TRY(h, dout.alloc(ds, hout.size() / 8));
      HIP_TRY(h, to_dev(din, hin));
      if (residual) HIP_TRY(h, to_dev(dout.p(), hres));
      HIP_TRY(h, hipDeviceSynchronize());
      const float* dres = residual ? reinterpret_cast<const float*>(dout.p()) : nullptr;
      SlotIn ls{din, 0, h_px, w};
      HIP_TRY(h, k == 5 ? (launch_conv_x3s<5, 2, 32, 4, 32, 32, 1, true, SlotIn>(st, L, ls, n, Ho, Wo, reinterpret_cast<float*>(dout.p()), dres, lrelu != 0, ncu, li))
                        : (launch_conv_x3s<3, 1, 32, 8, 16, 16, 2, true, SlotIn>(st, L, ls, n, Ho, Wo, reinterpret_cast<float*>(dout.p()), dres, lrelu != 0, ncu, li)));
      HIP_TRY(h, hipStreamSynchronize(st));
      HIP_TRY(h, from_dev(hout, dout.p()));
      SN_GUARD_CHECK(h, dout, "k_conv_x3s");
    }
    host_from_slots(hout, n, Ho, Wo, out);
    return SN_OK;
  }
  float* din = nullptr;
  Guarded<float> dout;          // starts as the 0xff pattern
  const size_t nin = (size_t)n * cin * h_px * w, nout = (size_t)n * kC * Ho * Wo;
  HIP_TRY(h, ds.alloc(&din, nin));
  HIP_TRY(h, dout.alloc(ds, nout));
  HIP_TRY(h, hipMemcpy(din, in, nin * 4, hipMemcpyHostToDevice));
  const float* dres = nullptr;
  if (residual) {   // in-place form, as the pipeline uses it
    HIP_TRY(h, hipMemcpy(dout.p(), residual, nout * 4, hipMemcpyHostToDevice));
    dres = dout.p();
  }
  HIP_TRY(h, hipDeviceSynchronize());
  LoadF32 ld{din, cin, h_px, w};
  hipError_t e;
  if (k == 5) {
    e = (Ho * Wo <= 64 * 128) ? launch_conv<5, 2, 1, 4, 4, 32>(st, L, ld, n, Ho, Wo, dout.p(), dres, lrelu != 0)
                              : launch_conv<5, 2, 1, 4, 8, 64>(st, L, ld, n, Ho, Wo, dout.p(), dres, lrelu != 0);
  } else if (cin <= 4) {
    if (dil != 1) return SN_ERR_ARG;
    e = (Ho * Wo <= 64 * 128) ? launch_conv<3, 1, 1, 4, 4, 32>(st, L, ld, n, Ho, Wo, dout.p(), dres, lrelu != 0)
                              : launch_conv<3, 1, 1, 4, 8, 64>(st, L, ld, n, Ho, Wo, dout.p(), dres, lrelu != 0);
  } else {
    if (tower32 && ((w & 3) != 0 || cin != kC)) return SN_ERR_ARG;
    e = conv3x3(st, L, din, n, h_px, w, dil, dout.p(), dres, lrelu != 0, tower32 ? ncu : 0, li);
  }
  HIP_TRY(h, e);
  HIP_TRY(h, hipStreamSynchronize(st));
  HIP_TRY(h, hipMemcpy(out, dout.p(), nout * 4, hipMemcpyDeviceToHost));
  SN_GUARD_CHECK(h, dout, "the fp32 convolution");
  return SN_OK;
}

int sn_dbg_down0_n(sn_handle* h, int n, const int8_t* in6, int h_px, int w, const float* wt, const float* bias, int tc,
                   float* out) {
  DevScope ds;      // frees every tracked device buffer on every return path
  if (!h || !in6 || !wt || !bias || !out || h_px <= 0 || w <= 0 || tc != 32 || n <= 0) return SN_ERR_ARG;
  int rc = check_device(h);
  if (rc) return rc;
  const int Hp = (h_px + 15) / 16 * 16, Wp = (w + 15) / 16 * 16, Ho = Hp / 2, Wo = Wp / 2;
  Down0F16 L;
  rc = upload_down0_f16(h, HostLayer{wt, bias, kC, 3, 25}, &L);
  ds.adopt(L);
  if (rc) return rc;
  int8_t* din = nullptr;
  float *dout = nullptr, *dbias = nullptr;
  const size_t nin = (size_t)n * 6 * h_px * w, nout = (size_t)n * 2 * kC * Ho * Wo;     // split slots: same bytes as fp32
  HIP_TRY(h, ds.alloc(&din, nin));
  HIP_TRY(h, ds.alloc(&dout, nout));
  HIP_TRY(h, ds.alloc(&dbias, kC));
  HIP_TRY(h, hipMemcpy(din, in6, nin, hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(dbias, bias, kC * 4, hipMemcpyHostToDevice));
  HIP_TRY(h, memset_now(dout, 0xff, nout * 4));       // an element the kernel does not write reads back as NaN
  HIP_TRY(h, launch_down0_f16(h->stream, L, dbias, din, h_px, w, 2 * n, Ho, Wo, dout, dbg_cus(h), nullptr, &h->dbg_launch));   // the pipeline's kernel
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  std::vector<_Float16> hs(nout * 2);
  HIP_TRY(h, from_dev(hs, dout));
  host_from_slots(hs, 2 * n, Ho, Wo, out);
  return SN_OK;
}

int sn_dbg_round_kernels_f16(const float* w, int nkernels, float* out) {
  if (!w || !out || nkernels < 0) return SN_ERR_ARG;
  for (int k = 0; k < nkernels; ++k) {          // host only: no device needed
    _Float16 q[9];
    round_kernel_sum_preserving(w + (size_t)k * 9, q);
    for (int t = 0; t < 9; ++t) out[(size_t)k * 9 + t] = (float)q[t];
  }
  return SN_OK;
}

int sn_dbg_compose_down01(const float* w0, const float* b0, const float* w1, const float* b1, float* weff, float* beff) {
  if (!w0 || !b0 || !w1 || !b1 || !weff || !beff) return SN_ERR_ARG;
  std::vector<double> we, be;
  compose_down01(w0, b0, w1, b1, we, be);         // host only: no device needed
  for (size_t i = 0; i < we.size(); ++i) weff[i] = (float)we[i];
  for (size_t i = 0; i < be.size(); ++i) beff[i] = (float)be[i];
  return SN_OK;
}

int sn_dbg_down01_n(sn_handle* h, int n, const int8_t* in6, int h_px, int w, const float* w0, const float* b0, const float* w1,
                    const float* b1, float* out) {
  DevScope ds;      // frees every tracked device buffer on every return path
  if (!h || !in6 || !w0 || !b0 || !w1 || !b1 || !out || h_px <= 0 || w <= 0 || n <= 0) return SN_ERR_ARG;
  SN_DBG_BANDED(h);
  int rc = check_device(h);
  if (rc) return rc;
  const int Hp = (h_px + 15) / 16 * 16, Wp = (w + 15) / 16 * 16, Ho = Hp / 4, Wo = Wp / 4;
  Down01W L;
  rc = upload_down01(h, HostLayer{w0, b0, kC, 3, 25}, HostLayer{w1, b1, kC, kC, 25}, &L);
  ds.adopt(L);
  if (rc) return rc;
  int8_t* din = nullptr;
  uint4* dout = nullptr;
  const size_t nin = (size_t)n * 6 * h_px * w, nout = (size_t)n * 2 * kC * Ho * Wo;     // split slots: same bytes as fp32
  HIP_TRY(h, ds.alloc(&din, nin));
  HIP_TRY(h, ds.alloc(&dout, nout / 4));
  HIP_TRY(h, hipMemcpy(din, in6, nin, hipMemcpyHostToDevice));
  HIP_TRY(h, memset_now(dout, 0xff, nout * 4));       // an element neither kernel writes reads back as NaN
  HIP_TRY(h, launch_down01(h->stream, L, din, h_px, w, 2 * n, Ho, Wo, dout, SlotGeom{Ho, Wo, 0, 0}, dbg_cus(h), &h->dbg_launch));   // the pipeline's kernels
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  std::vector<_Float16> hs(nout * 2);
  HIP_TRY(h, from_dev(hs, dout));
  host_from_slots(hs, 2 * n, Ho, Wo, out);
  return SN_OK;
}

int sn_dbg_refin_n(sn_handle* h, int n, const float* disp_low, const int8_t* in6, int h_px, int w, int dmax, const float* wt,
                   const float* bias, int split, float* out) {
  if (h_px <= 0 || w <= 0 || dmax <= 0) return SN_ERR_ARG;
  const int Hp = (h_px + 15) / 16 * 16, Wp = (w + 15) / 16 * 16, hl = Hp / 16, wl = Wp / 16;
  TowerHook th(h, "ref.in");
  // no tower tensor to read, and [hi | slack | lo | slack] whatever `split` says
  int rc = th.begin({disp_low, in6, wt, bias, out}, n, Hp, Wp, 1, kTowerSplit | (split ? 0 : kTowerHiOnly), nullptr, nullptr, {});
  if (rc) return rc;
  Down0F16 L;
  rc = upload_refin_f16(h, HostLayer{wt, bias, kC, 4, 9}, &L);
  th.ds.adopt(L);
  if (rc) return rc;
  float *ddl = nullptr, *dbias = nullptr;
  int8_t* din = nullptr;
  HIP_TRY(h, th.ds.alloc(&ddl, (size_t)n * hl * wl));
  HIP_TRY(h, th.ds.alloc(&dbias, kC));
  HIP_TRY(h, th.ds.alloc(&din, (size_t)n * 6 * h_px * w));
  HIP_TRY(h, hipMemcpy(ddl, disp_low, (size_t)n * hl * wl * 4, hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(dbias, bias, kC * 4, hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(din, in6, (size_t)n * 6 * h_px * w, hipMemcpyHostToDevice));
  return th.run(out, [&] {
    return launch_refin_f16(h->stream, L, dbias, ddl, din, false, hl, wl, h_px, w, 1.0f / (float)dmax, UpScale{1.0f / 16.0f, 16.0f},
                            th.t.g, n, th.y.base, split != 0, th.t.lo_slots * 16, dbg_cus(h), &h->dbg_launch);
  });
}

int sn_dbg_conv3d(sn_handle* h, const float* in, int d, int h_px, int w, const float* wt, const float* bias,
                  int lrelu, int form, float* out) {
  DevScope ds;      // frees every tracked device buffer on every return path
  if (!h || !in || !wt || !bias || !out || d <= 0) return SN_ERR_ARG;
  int rc = check_device(h);
  if (rc) return rc;
  if (form != SN_DBG_CONV_F32 && form != SN_DBG_CONV_SLOTS && form != SN_DBG_CONV_SLOTS_DMA) return SN_ERR_ARG;
  const bool dma = form == SN_DBG_CONV_SLOTS_DMA, slots = dma || form == SN_DBG_CONV_SLOTS;
  if (slots) SN_DBG_BANDED(h);
  h->dbg_launch = LaunchInfo{};
  ConvLayer L;
  rc = upload_conv3d(h, HostLayer{wt, bias, kC, kC, 27}, &L);
  if (!rc && slots)
    rc = upload_x3(h, 96, [&](int co, int c, int tap) { return wt[(((size_t)co * kC + (c & 31)) * 3 + (c >> 5)) * 9 + tap]; }, &L);
  ds.adopt(L);
  if (rc) return rc;
  const size_t plane = (size_t)h_px * w, n = (size_t)kC * d * plane;
  // caller layout [ci][d][h][w] (PyTorch) <-> device layout [d][ci][h][w]
  std::vector<float> tmp(n);
  for (int ci = 0; ci < kC; ++ci)
    for (int z = 0; z < d; ++z)
      memcpy(&tmp[((size_t)z * kC + ci) * plane], &in[((size_t)ci * d + z) * plane], plane * 4);
  float *din = nullptr, *dout = nullptr;
  HIP_TRY(h, ds.alloc(&din, n));
  HIP_TRY(h, ds.alloc(&dout, n));
  if (slots) {       // the volume as d split-slot images (same byte count as fp32)
    std::vector<_Float16> hs, ho(n * 2);
    host_to_slots(tmp.data(), d, h_px, w, hs);
    if (dma) {         // k_agg_x3s_dma on the padded layout: planes 1 .. d of d + 2, every (block, part) image with its border
      const VolPad g = vol_pad(d, h_px, w);
      PaddedSlots pin(SlotGeom{g.PH, g.PW, 1, 1}, h_px, w, (size_t)d * 8, 8), pout = pin;
      pin.put(hs);
      memset(ho.data(), 0xff, ho.size() * 2);
      pout.put(ho);                                // 0xff inside the images, zeros everywhere else
      uint4 *pdin = nullptr, *pdout = nullptr;
      HIP_TRY(h, ds.alloc(&pdin, pin.v.size() / 8));
      HIP_TRY(h, ds.alloc(&pdout, pout.v.size() / 8));
      HIP_TRY(h, to_dev(pdin, pin.v));
      HIP_TRY(h, to_dev(pdout, pout.v));
      HIP_TRY(h, hipDeviceSynchronize());
      HIP_TRY(h, launch_agg_dma<true>(h->stream, L, pdin, g, 1, pdout, lrelu != 0, dbg_cus(h), nullptr, &h->dbg_launch));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      HIP_TRY(h, from_dev(pout.v, pdout));
      pout.get(ho);
      if (!pout.outside_is_zero()) {      // the borders must still hold the zeros of the allocation
        set_err(h, "k_agg_x3s_dma wrote outside the image");
        return SN_ERR_DEVICE;
      }
    } else {
      HIP_TRY(h, to_dev(din, hs));
      SlotIn ls{reinterpret_cast<const uint4*>(din), d, h_px, w};
      HIP_TRY(h, memset_now(dout, 0xff, n * 4));
      HIP_TRY(h, (launch_conv_x3s<3, 1, 96, 8, 16, 16, 1, true, SlotIn>(h->stream, L, ls, d, h_px, w, dout, nullptr, lrelu != 0, dbg_cus(h), &h->dbg_launch)));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      HIP_TRY(h, from_dev(ho, dout));
    }
    host_from_slots(ho, d, h_px, w, tmp.data());
  } else {
    HIP_TRY(h, to_dev(din, tmp));
    LoadVol3D lv{din, d, h_px, w};
    HIP_TRY(h, (launch_conv<3, 1, 1, 8, 4, 32>(h->stream, L, lv, d, h_px, w, dout, nullptr, lrelu != 0)));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, from_dev(tmp, dout));
  }
  for (int co = 0; co < kC; ++co)
    for (int z = 0; z < d; ++z)
      memcpy(&out[((size_t)co * d + z) * plane], &tmp[((size_t)z * kC + co) * plane], plane * 4);
  return SN_OK;
}

int sn_dbg_ref_conv_f16_n(sn_handle* h, int n, const float* in, int h_px, int w, const float* wt, const float* bias, int dil,
                          int lrelu, int tile_w, const float* residual, float* out) {
  if (tile_w != 0 && tile_w != 64 && tile_w != 32) return SN_ERR_ARG;
  TowerHook th(h, "the fp16 conv");
  const int rc = th.begin({in, wt, bias, out}, n, h_px, w, dil, kTowerBanded | kTowerQueue, in, residual, {{wt, bias}});
  if (rc) return rc;
  return th.run(out, [&] {
    return ref_conv_f16(h->stream, th.L[0], th.t.g, dbg_cus(h), dil, th.x.base, th.y.base, residual ? th.y.base : nullptr, n,
                        lrelu != 0, h->ws.tile_ctr, tile_w, &h->dbg_launch);
  });
}

int sn_dbg_ref_conv_f16x3_n(sn_handle* h, int n, const float* in, int h_px, int w, const float* wt, const float* bias, int dil,
                            int lrelu, const float* residual, float* out) {
  TowerHook th(h, "the f16x3 conv");
  const int rc = th.begin({in, wt, bias, out}, n, h_px, w, dil, kTowerSplit | kTowerBanded, in, residual, {{wt, bias}});
  if (rc) return rc;
  return th.run(out, [&] {
    return ref_conv_f16x3(h->stream, th.L[0], th.t.g, dbg_cus(h), dil, th.x.base, th.y.base, residual ? th.y.base : nullptr,
                          th.t.lo_slots, n, lrelu != 0, &h->dbg_launch);
  });
}

// The block launchers take the input in *cur, use *oth as they see fit and leave the result in *cur: th.res is that cur.
int sn_dbg_ref_block_f16x3_n(sn_handle* h, int n, const float* in, int h_px, int w, const float* w1, const float* b1,
                             const float* w2, const float* b2, int dil, int form, float* out) {
  if ((form != 0 && form != 1) || (form == 1 && !stream_x3_supports(dil))) return SN_ERR_ARG;
  TowerHook th(h, "the f16x3 residual block");
  const int rc = th.begin({in, w1, b1, w2, b2, out}, n, h_px, w, dil, kTowerSplit | (form == 0 ? kTowerBanded : 0), in, nullptr,
                          {{w1, b1}, {w2, b2}});
  if (rc) return rc;
  return th.run(out, [&] {
    uint4* oth = th.y.base;
    th.res = th.x.base;
    return ref_block_f16x3(h->stream, th.L[0], th.L[1], th.t.g, dbg_cus(h), dil, &th.res, &oth, th.t.lo_slots, n, form == 1,
                           &h->dbg_launch);
  });
}

int sn_dbg_ref_block_f16_n(sn_handle* h, int n, const float* in, int h_px, int w, const float* w1, const float* b1,
                           const float* w2, const float* b2, int dil, int form, float* out) {
  if ((form != 0 && form != 1) || (form == 1 && !stream_block_supports(dil))) return SN_ERR_ARG;
  TowerHook th(h, "the fp16 residual block");
  const int rc = th.begin({in, w1, b1, w2, b2, out}, n, h_px, w, dil, kTowerQueue | (form == 0 ? kTowerBanded : 0), in, nullptr,
                          {{w1, b1}, {w2, b2}});
  if (rc) return rc;
  return th.run(out, [&] {
    uint4* oth = th.y.base;
    th.res = th.x.base;
    return ref_block_f16(h->stream, th.L[0], th.L[1], th.t.g, dbg_cus(h), dil, &th.res, &oth, n, h->ws.tile_ctr, form == 1 ? 4 : 0,
                         h->dump, false, &h->dbg_launch);
  });
}

int sn_dbg_ref_tail_f16(sn_handle* h, int n, const float* in, int hk, int wk, const float* w1, const float* b1, const float* w2,
                        const float* b2, const float* head_w, float head_b, const float* low, int ups, float dnorm, int h_out,
                        int w_out, int form, float* out_disp, int32_t* out_raw) {
  if (!h || !head_w || h_out <= 0 || w_out <= 0 || h_out > hk || w_out > wk || (ups != 16 && ups != 2) || hk % ups || wk % ups ||
      (form != 0 && form != 1) || !(dnorm > 0.f))
    return SN_ERR_ARG;
  if (h->precision != SN_PREC_F16 && h->precision != SN_PREC_AUTO) {
    set_err(h, "sn_dbg_ref_tail_f16 needs an engine created with SN_PREC_F16 or SN_PREC_AUTO");
    return SN_ERR_ARG;
  }
  // y: written by form 0 only
  TowerHook th(h, form == 1 ? "the tail form (the tensor it must not write)" : "the streamed block in front of the head",
               "the tail (its input tensor)");
  int rc = th.begin({in, w1, b1, w2, b2, low, out_disp, out_raw}, n, hk, wk, 1, 0, in, nullptr, {{w1, b1}, {w2, b2}});
  if (rc) return rc;
  HeadLayer hd;
  rc = upload_head(h, HostLayer{head_w, &head_b, 1, kC, 9}, &hd);
  th.ds.adopt(hd);
  if (rc) return rc;
  const int sh = hk / ups, sw = wk / ups;
  const size_t nlow = (size_t)n * sh * sw, nout = (size_t)n * h_out * w_out;
  float *dlow = nullptr, *dd = nullptr;
  int32_t* dr = nullptr;
  HIP_TRY(h, th.ds.alloc(&dlow, nlow));
  HIP_TRY(h, th.ds.alloc(&dd, nout));
  HIP_TRY(h, th.ds.alloc(&dr, nout));
  HIP_TRY(h, hipMemcpy(dlow, low, nlow * 4, hipMemcpyHostToDevice));
  HIP_TRY(h, memset_now(dd, 0xff, nout * 4));        // NaN / -1: a pixel the kernel does not write shows up
  HIP_TRY(h, memset_now(dr, 0xff, nout * 4));
  const float inv_q = (float)(1.0 / (kWireFactor * (double)kOutScale));
  const UpScale us{1.0f / (float)ups, (float)ups};
  const HeadArgs ha{hd.w, dlow, dd, dr, hd.bias, dnorm, inv_q, sh, sw, h_out, w_out, us};
  rc = th.run(nullptr, [&]() -> hipError_t {
    if (form == 1) return ref_block_stream_tail(h->stream, th.L[0], th.L[1], th.t.g, dbg_cus(h), th.x.base, n, h->dump, ha, &h->dbg_launch);
    const hipError_t e = ref_block_stream(h->stream, th.L[0], th.L[1], th.t.g, dbg_cus(h), 1, th.x.base, th.y.base, n, h->dump, &h->dbg_launch);
    return e != hipSuccess ? e : launch_head_final_f16(h->stream, false, th.y.base, 0, th.t.g, n, ha);
  });
  if (rc) return rc;
  HIP_TRY(h, hipMemcpy(out_disp, dd, nout * 4, hipMemcpyDeviceToHost));
  HIP_TRY(h, hipMemcpy(out_raw, dr, nout * 4, hipMemcpyDeviceToHost));
  return SN_OK;
}

// ---- mid-stage hooks: cost volume, aggregation tail, soft-argmin, refinement heads, image pyramid -------------------
// Each runs the kernel through the launch code of the forward pass on caller tensors; every device output sits between
// guard bands (Guarded) and starts as the 0xff pattern, padded layouts are checked with PaddedSlots::outside_is_zero.
int sn_dbg_cost_volume(sn_handle* h, const float* feat, int n, int Dl, int hl, int wl, int form, float* out) {
  DevScope ds;
  if (!h || !feat || !out || n <= 0 || Dl <= 0 || hl <= 0 || wl <= 0 || (form != 0 && form != 1)) return SN_ERR_ARG;
  int rc = check_device(h);
  if (rc) return rc;
  const size_t plane = (size_t)hl * wl, nfeat = (size_t)2 * n * kC * plane;
  float* dfeat = nullptr;
  HIP_TRY(h, ds.alloc(&dfeat, nfeat));
  HIP_TRY(h, hipMemcpy(dfeat, feat, nfeat * 4, hipMemcpyHostToDevice));
  std::vector<_Float16> hs((size_t)n * Dl * 8 * plane * 8);
  Guarded<uint4> dvol;
  if (form == 0) {
    HIP_TRY(h, dvol.alloc(ds, hs.size() / 8));
    HIP_TRY(h, launch_cost_slots(h->stream, dfeat, dvol.p(), Dl, hl, wl, n));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, from_dev(hs, dvol.p()));
  } else {
    const VolPad g = vol_pad(Dl, hl, wl);
    PaddedSlots pv = vol_padded(g, n);
    memset(hs.data(), 0xff, hs.size() * 2);
    pv.put(hs);                                  // 0xff inside the images, zeros everywhere else
    HIP_TRY(h, dvol.alloc(ds, pv.v.size() / 8));
    HIP_TRY(h, to_dev(dvol.p(), pv.v));
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, launch_cost_slots_pad(h->stream, dfeat, dvol.p(), g, n));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, from_dev(pv.v, dvol.p()));
    pv.get(hs);
    if (!pv.outside_is_zero()) {
      set_err(h, "k_cost_slots_pad wrote outside the image");
      return SN_ERR_DEVICE;
    }
  }
  SN_GUARD_CHECK(h, dvol, form == 0 ? "k_cost_slots" : "k_cost_slots_pad");
  host_from_slots(hs, n * Dl, hl, wl, out);
  return SN_OK;
}

int sn_dbg_agg_first_f32(sn_handle* h, const float* feat, int n, int Dl, int hl, int wl, const float* wt, const float* bias,
                         float* out) {
  DevScope ds;
  if (!h || !feat || !wt || !bias || !out || n <= 0 || Dl <= 0 || hl <= 0 || wl <= 0) return SN_ERR_ARG;
  int rc = check_device(h);
  if (rc) return rc;
  ConvLayer L;
  rc = upload_conv3d(h, HostLayer{wt, bias, kC, kC, 27}, &L);
  ds.adopt(L);
  if (rc) return rc;
  const size_t plane = (size_t)hl * wl, nfeat = (size_t)2 * n * kC * plane, nout = (size_t)n * Dl * kC * plane;
  float* dfeat = nullptr;
  Guarded<float> dout;
  HIP_TRY(h, ds.alloc(&dfeat, nfeat));
  HIP_TRY(h, dout.alloc(ds, nout));
  HIP_TRY(h, hipMemcpy(dfeat, feat, nfeat * 4, hipMemcpyHostToDevice));
  LoadCostVol ld{dfeat, Dl, hl, wl};
  HIP_TRY(h, (launch_conv<3, 1, 1, 8, 4, 32>(h->stream, L, ld, n * Dl, hl, wl, dout.p(), nullptr, true)));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipMemcpy(out, dout.p(), nout * 4, hipMemcpyDeviceToHost));
  SN_GUARD_CHECK(h, dout, "the fp32 first aggregation layer");
  return SN_OK;
}

int sn_dbg_softargmin(sn_handle* h, int n, int Dl, int hl, int wl, int form, int want_conf, float bias, const float* v,
                      const float* w, float* cost, float* disp_low, float* conf_low, unsigned long long* nonfinite) {
  DevScope ds;
  if (!h || !v || !cost || !disp_low || !nonfinite || n <= 0 || Dl <= 0 || Dl > 16 || hl <= 0 || wl <= 0) return SN_ERR_ARG;
  if ((form != 0 && form != 1) || (form == 0 && !w) || (want_conf && !conf_low)) return SN_ERR_ARG;
  int rc = check_device(h);
  if (rc) return rc;
  const size_t plane = (size_t)hl * wl, npix = (size_t)n * plane, nv = npix * Dl * (form == 0 ? kC : 27);
  float *dv = nullptr, *dw = nullptr;
  Guarded<float> dcost, ddisp, dconf;
  HookStat st;
  HIP_TRY(h, ds.alloc(&dv, nv));
  HIP_TRY(h, hipMemcpy(dv, v, nv * 4, hipMemcpyHostToDevice));
  if (form == 0) {
    HIP_TRY(h, ds.alloc(&dw, (size_t)kC * 27));
    HIP_TRY(h, hipMemcpy(dw, w, (size_t)kC * 27 * 4, hipMemcpyHostToDevice));
  }
  HIP_TRY(h, dcost.alloc(ds, npix * Dl));
  HIP_TRY(h, ddisp.alloc(ds, npix));
  HIP_TRY(h, dconf.alloc(ds, npix));
  HIP_TRY(h, st.alloc(ds));
  HIP_TRY(h, launch_softargmin_kernels(h->stream, dv, form == 1, dw, bias, Dl, hl, wl, (int)npix, ddisp.p(), dcost.p(),
                                       want_conf ? dconf.p() : nullptr, st.dev + kStatNonfiniteLow));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipMemcpy(cost, dcost.p(), npix * Dl * 4, hipMemcpyDeviceToHost));
  HIP_TRY(h, hipMemcpy(disp_low, ddisp.p(), npix * 4, hipMemcpyDeviceToHost));
  if (conf_low) HIP_TRY(h, hipMemcpy(conf_low, dconf.p(), npix * 4, hipMemcpyDeviceToHost));     // !want_conf: still the 0xff pattern
  HIP_TRY(h, st.read(kStatNonfiniteLow, nonfinite));
  const char* const name = form == 1 ? "k_softargmin_p" : "k_head_softargmin";
  SN_GUARD_CHECK(h, dcost, name);
  SN_GUARD_CHECK(h, ddisp, name);
  SN_GUARD_CHECK(h, dconf, name);
  return SN_OK;
}

int sn_dbg_agg_tail(sn_handle* h, const float* vol, int n, int Dl, int hl, int wl, const float* wt, const float* bias,
                    const float* out_w, float out_b, int form, int want_conf, float* cost, float* disp_low, float* conf_low,
                    unsigned long long* nonfinite, float* layer_vol) {
  DevScope ds;
  if (!h || !vol || !wt || !bias || !out_w || !cost || !disp_low || !nonfinite || n <= 0 || Dl <= 0 || Dl > 16 || hl <= 0 ||
      wl <= 0 || form < 0 || form > 2 || (want_conf && !conf_low) || (form == 2 && layer_vol))
    return SN_ERR_ARG;
  SN_DBG_BANDED(h);
  int rc = check_device(h);
  if (rc) return rc;
  ConvLayer L;
  HeadLayer hd;
  rc = upload_conv3d(h, HostLayer{wt, bias, kC, kC, 27}, &L);
  if (!rc) rc = upload_x3(h, 96, [&](int co, int c, int tap) { return wt[(((size_t)co * kC + (c & 31)) * 3 + (c >> 5)) * 9 + tap]; }, &L);
  if (!rc) rc = upload_head(h, HostLayer{out_w, &out_b, 1, kC, 27}, &hd);
  if (!rc && form == 2) rc = upload_agg_head_frag(h, HostLayer{out_w, &out_b, 1, kC, 27}, &hd);
  ds.adopt(L);
  ds.adopt(hd);
  if (rc) return rc;
  const size_t plane = (size_t)hl * wl, npix = (size_t)n * plane;
  const size_t nmid = npix * Dl * (form == 2 ? 27 : kC);       // the layer's fp32 output: volume, or the partial sums P
  std::vector<float> tmp;
  vol_to_device_order(vol, n, Dl, plane, tmp);
  std::vector<_Float16> hs;
  host_to_slots(tmp.data(), n * Dl, hl, wl, hs);
  uint4* din = nullptr;
  Guarded<float> dmid, dcost, ddisp, dconf;
  HookStat st;
  HIP_TRY(h, dmid.alloc(ds, nmid));
  HIP_TRY(h, dcost.alloc(ds, npix * Dl));
  HIP_TRY(h, ddisp.alloc(ds, npix));
  HIP_TRY(h, dconf.alloc(ds, npix));
  HIP_TRY(h, st.alloc(ds));
  if (form == 0) {
    HIP_TRY(h, ds.alloc(&din, hs.size() / 8));
    HIP_TRY(h, to_dev(din, hs));
    HIP_TRY(h, hipDeviceSynchronize());
    SlotIn ls{din, Dl, hl, wl};
    HIP_TRY(h, (launch_conv_x3s<3, 1, 96, 8, 16, 16, 1, false, SlotIn>(h->stream, L, ls, n * Dl, hl, wl, dmid.p(), nullptr, true, dbg_cus(h))));
  } else {
    const VolPad g = vol_pad(Dl, hl, wl);
    PaddedSlots pin = vol_padded(g, n);
    pin.put(hs);
    HIP_TRY(h, ds.alloc(&din, pin.v.size() / 8));
    HIP_TRY(h, to_dev(din, pin.v));
    HIP_TRY(h, hipDeviceSynchronize());
    if (form == 1)
      HIP_TRY(h, launch_agg_dma<false>(h->stream, L, din, g, n, dmid.p(), true, dbg_cus(h)));
    else
      HIP_TRY(h, (launch_agg_dma<false, true>(h->stream, L, din, g, n, dmid.p(), true, dbg_cus(h), hd.pfrag)));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, from_dev(pin.v, din));
    if (!pin.outside_is_zero()) {      // the padded volume is this layer's input only: its borders still hold the zeros
      set_err(h, "k_agg_x3s_dma (fp32 output) wrote into the padded input volume");
      return SN_ERR_DEVICE;
    }
  }
  HIP_TRY(h, launch_softargmin_kernels(h->stream, dmid.p(), form == 2, hd.w, hd.bias, Dl, hl, wl, (int)npix, ddisp.p(), dcost.p(),
                                       want_conf ? dconf.p() : nullptr, st.dev + kStatNonfiniteLow));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipMemcpy(cost, dcost.p(), npix * Dl * 4, hipMemcpyDeviceToHost));
  HIP_TRY(h, hipMemcpy(disp_low, ddisp.p(), npix * 4, hipMemcpyDeviceToHost));
  if (conf_low) HIP_TRY(h, hipMemcpy(conf_low, dconf.p(), npix * 4, hipMemcpyDeviceToHost));
  if (layer_vol) HIP_TRY(h, hipMemcpy(layer_vol, dmid.p(), nmid * 4, hipMemcpyDeviceToHost));      // [n Dl][32][hl][wl]
  HIP_TRY(h, st.read(kStatNonfiniteLow, nonfinite));
  SN_GUARD_CHECK(h, dmid, form == 0 ? "k_conv_x3s (fp32 output)" : "k_agg_x3s_dma (fp32 output)");
  SN_GUARD_CHECK(h, dcost, "the soft-argmin");
  SN_GUARD_CHECK(h, ddisp, "the soft-argmin");
  SN_GUARD_CHECK(h, dconf, "the soft-argmin");
  return SN_OK;
}

int sn_dbg_head(sn_handle* h, int n, const float* x, int hk, int wk, const float* head_w, float head_b, const float* low, int ups,
                float dnorm, int h_out, int w_out, int form, float* out_disp, int32_t* out_raw, double* mean_abs_dr,
                unsigned long long* nonfinite) {
  DevScope ds;
  if (!h || !x || !head_w || !low || !out_disp || !out_raw || !mean_abs_dr || !nonfinite) return SN_ERR_ARG;
  if (n <= 0 || hk <= 0 || wk <= 0 || h_out <= 0 || w_out <= 0 || h_out > hk || w_out > wk || (ups != 16 && ups != 2) ||
      hk % ups || wk % ups || form < 0 || form > 2 || !(dnorm > 0.f))
    return SN_ERR_ARG;
  if (form != 2 && h->precision != SN_PREC_FP32) {
    set_err(h, "sn_dbg_head forms 0 and 1 need an engine created with SN_PREC_FP32");
    return SN_ERR_ARG;
  }
  if (form == 2 && h->precision == SN_PREC_FP32) {
    set_err(h, "sn_dbg_head form 2 needs an engine created in an fp16 mode");
    return SN_ERR_ARG;
  }
  int rc = check_device(h);
  if (rc) return rc;
  HeadLayer hd;
  rc = form == 2 ? upload_head_split(h, HostLayer{head_w, &head_b, 1, kC, 9}, &hd) : upload_head(h, HostLayer{head_w, &head_b, 1, kC, 9}, &hd);
  ds.adopt(hd);
  if (rc) return rc;
  const int sh = hk / ups, sw = wk / ups;
  const size_t nlow = (size_t)n * sh * sw, nout = (size_t)n * h_out * w_out;
  float* dlow = nullptr;
  Guarded<float> dd;
  Guarded<int32_t> dr;
  HookStat st;
  HIP_TRY(h, ds.alloc(&dlow, nlow));
  HIP_TRY(h, dd.alloc(ds, nout));
  HIP_TRY(h, dr.alloc(ds, nout));
  HIP_TRY(h, st.alloc(ds));
  HIP_TRY(h, hipMemcpy(dlow, low, nlow * 4, hipMemcpyHostToDevice));
  const float inv_q = (float)(1.0 / (kWireFactor * (double)kOutScale));
  const UpScale us{1.0f / (float)ups, (float)ups};
  if (form == 2) {        // the split head of SN_PREC_F16X3 on the hi / lo tower tensor, as refine_level launches it
    const RefGeom g = make_ref_geom(hk, wk);
    if ((2 * (ref16_slots(g, n) + ref_slack(g)) + ref_front(g)) * 16 >= ((size_t)1 << 32)) return SN_ERR_ARG;
    RefHost t(g, n, hk, wk, true, true);      // [hi | slack | lo | slack]
    t.pack(x, true);
    uint4* da = nullptr;
    HIP_TRY(h, alloc_ref16(ds, g, t.slots(), &da));
    HIP_TRY(h, to_dev(da, t.v));
    HIP_TRY(h, hipDeviceSynchronize());
    const HeadArgs ha{hd.wsplit, dlow, dd.p(), dr.p(), hd.biassplit, dnorm * hd.unscale, inv_q, sh, sw, h_out, w_out, us, st.dev};
    HIP_TRY(h, launch_head_final_f16(h->stream, true, da, t.lo_slots, g, n, ha));
  } else {
    const size_t nx = (size_t)n * kC * hk * wk;
    float* dx = nullptr;
    HIP_TRY(h, ds.alloc(&dx, nx));
    HIP_TRY(h, hipMemcpy(dx, x, nx * 4, hipMemcpyHostToDevice));
    const HeadArgs ha{hd.w, dlow, dd.p(), dr.p(), hd.bias, dnorm, inv_q, sh, sw, h_out, w_out, us, st.dev};
    HIP_TRY(h, launch_head_final_f32(h->stream, form == 1, dx, hk, wk, n, ha));
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipMemcpy(out_disp, dd.p(), nout * 4, hipMemcpyDeviceToHost));
  HIP_TRY(h, hipMemcpy(out_raw, dr.p(), nout * 4, hipMemcpyDeviceToHost));
  unsigned long long sum = 0;
  HIP_TRY(h, st.read(0, &sum));
  HIP_TRY(h, st.read(kStatNonfinite, nonfinite));
  *mean_abs_dr = (double)sum / (double)kStatScale / (double)nout;
  const char* const name = form == 0 ? "k_head_final" : form == 1 ? "k_head_final_mfma32" : "k_head_final_f16<true>";
  SN_GUARD_CHECK(h, dd, name);
  SN_GUARD_CHECK(h, dr, name);
  return SN_OK;
}

int sn_dbg_img_pool2(sn_handle* h, const int8_t* in6, int n, int h_px, int w, int levels, float* out) {
  DevScope ds;
  if (!h || !in6 || !out || n <= 0 || h_px <= 0 || w <= 0 || levels < 2 || levels > kMaxLevels) return SN_ERR_ARG;
  int rc = check_device(h);
  if (rc) return rc;
  const int Hp = (h_px + 15) / 16 * 16, Wp = (w + 15) / 16 * 16;
  const size_t nin = (size_t)n * 6 * h_px * w;
  int8_t* din = nullptr;
  HIP_TRY(h, ds.alloc(&din, nin));
  HIP_TRY(h, hipMemcpy(din, in6, nin, hipMemcpyHostToDevice));
  Guarded<float> lvl[kMaxLevels];
  for (int lv = 1; lv < levels; ++lv) HIP_TRY(h, lvl[lv].alloc(ds, (size_t)n * 3 * (Hp >> lv) * (Wp >> lv)));
  for (int lv = 1; lv < levels; ++lv) {       // chained as refine_coarse chains them
    if (lv == 1)
      HIP_TRY(h, launch_img_pool2(h->stream, true, din, h_px, w, Hp >> lv, Wp >> lv, lvl[lv].p(), n));
    else
      HIP_TRY(h, launch_img_pool2(h->stream, false, lvl[lv - 1].p(), 0, 0, Hp >> lv, Wp >> lv, lvl[lv].p(), n));
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int lv = 1; lv < levels; ++lv) {
    const size_t cnt = (size_t)n * 3 * (Hp >> lv) * (Wp >> lv);
    HIP_TRY(h, hipMemcpy(out, lvl[lv].p(), cnt * 4, hipMemcpyDeviceToHost));
    out += cnt;
    SN_GUARD_CHECK(h, lvl[lv], "k_img_pool2");
  }
  return SN_OK;
}

// The fp32 coefficients of k_jpeg_dct before quantisation for one host NV12 image: out [blocks][64], coefficient (v, u) of a
// block at u * 8 + v (the layout the host encoder's two passes leave)
int sn_dbg_jpeg_dct(sn_handle* h, const uint8_t* nv12, int w, int h_px, int pitch, float* out) {
  DevScope ds;      // frees every tracked device buffer on every return path
  if (!h || !nv12 || !out || !jpg_size_ok(w, h_px) || pitch < w) return SN_ERR_ARG;
  int rc = check_device(h);
  if (rc) return rc;
  const size_t span = (size_t)(h_px + h_px / 2 - 1) * pitch + w;
  const size_t blocks = (size_t)((w + 15) / 16) * jpg_mcu_rows(h_px) * 6;
  JpgPlan plan;
  jpg_make_plan(w, h_px, 50, 0, &plan);
  uint8_t* din = nullptr;
  int16_t* dcoef = nullptr;
  float* ddct = nullptr;
  HIP_TRY(h, ds.alloc(&din, span));
  HIP_TRY(h, ds.alloc(&dcoef, blocks * 64));
  HIP_TRY(h, ds.alloc(&ddct, blocks * 64));
  HIP_TRY(h, hipMemcpy(din, nv12, span, hipMemcpyHostToDevice));
  if ((rc = jpeg_launch(h, h->stream, plan, 1, din, pitch, 0, 0, dcoef, nullptr, nullptr, nullptr, 0, nullptr, ddct))) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipMemcpy(out, ddct, blocks * 64 * 4, hipMemcpyDeviceToHost));
  return SN_OK;
}

__global__ __launch_bounds__(256) void k_copy_limited(uint4* __restrict__ dst, const uint4* __restrict__ src, size_t n16) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

int sn_dbg_copy_limited(void* dst, const void* src, size_t bytes, int workgroups, void* stream) {
  if (!dst || !src || (bytes & 15) || workgroups <= 0 || workgroups > 65535 || ((uintptr_t)dst & 15) || ((uintptr_t)src & 15)) return SN_ERR_ARG;
  hipLaunchKernelGGL(k_copy_limited, dim3((unsigned)workgroups), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<uint4*>(dst), static_cast<const uint4*>(src), bytes / 16);
  return hipGetLastError() == hipSuccess ? SN_OK : SN_ERR_DEVICE;
}

int sn_dbg_read(sn_handle* h, const char* what, float* dst, size_t cap, size_t* n) {
  if (!h || !what || !n) return SN_ERR_ARG;
  int rc = check_device(h);
  if (rc) return rc;
  const size_t hw = (size_t)h->hl * h->wl;
  const float* src = nullptr;
  size_t cnt = 0;
  if (!strcmp(what, "stream_prio")) {      // host state: 1 = the pipeline streams were created with the highest priority
    *n = 1;
    if (dst && cap >= 1) dst[0] = h->stream_prio ? 1.f : 0.f;
    return (dst && cap < 1) ? SN_ERR_ARG : SN_OK;
  }
  if (!strcmp(what, "feat_l")) { src = h->ws.feat; cnt = kC * hw; }
  else if (!strcmp(what, "feat_r")) { src = h->ws.feat + kC * hw; cnt = kC * hw; }
  else if (!strcmp(what, "cost")) { src = h->ws.cost; cnt = h->Dl * hw; }
  else if (!strcmp(what, "disp_low")) { src = h->ws.disp_low; cnt = hw; }
  else if (!strcmp(what, "conf_low")) { src = h->ws.conf_low; cnt = hw; }      // first pair of the last sn_infer_conf; other calls leave it alone (zeros before the first)
  else if (!strcmp(what, "tile_ctr") && h->ws.tile_ctr) { src = reinterpret_cast<const float*>(h->ws.tile_ctr); cnt = kTileCtrBytes / 4 * h->ws.n_chunks; }
  else if (!strcmp(what, "refine_x") && h->precision == SN_PREC_FP32) { src = h->ws.ref[0]; cnt = (size_t)kC * h->Hp * h->Wp; }
  else if (!strncmp(what, "level", 5) && what[5] >= '1' && what[5] < '0' + h->levels && what[6] == 0) {
    // hierarchical refinement: the map of level k (first pair of the last piece)
    const int k = what[5] - '0';
    src = h->ws.lvl_disp[k];
    cnt = (size_t)h->tw[k].Hk * h->tw[k].Wk;
  }
  else return SN_ERR_ARG;
  *n = cnt;
  if (!dst) return SN_OK;
  if (cap < cnt) return SN_ERR_ARG;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipMemcpy(dst, src, cnt * 4, hipMemcpyDeviceToHost));
  return SN_OK;
}

}  // extern "C"
