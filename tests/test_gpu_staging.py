"""The host staging the post-processing entry points share (csrc/sn_postproc.hpp) on the MI355X: ONE handle's grow-only
buffers — the inference stream's and every lane's, the temporal filter's and the rectifier's among them — used by different
entry points in growing and shrinking order, inference interleaved with the other calls, and device mode followed by host mode.  Every result equals its numpy twin (or a fresh handle's result) bit for bit: a stale
capacity, a slot shared by two meanings or a download of the previous call's size would show up as a wrong map.
96x64 takes the vector paths, 33x47 (W % 4 != 0, odd height) the scalar ones."""
import numpy as np
import pytest

from hobot_stereonet_amd import api, confidence, dispfilter, lrcheck, pointcloud, rectify, smooth, synth, temporal

SHAPES = [(96, 64), (33, 47)]
DMAX = 48
S = float(lrcheck.wire_scale())
S32 = dispfilter.wire_scale()
FLT = (6, 1.0, 16)               # speckle_max_px, speckle_diff_px, fill_max_px: both passes of the filter
SMO = (2, 12, 3)                 # radius, sigma_luma, min_valid: the weighted median, with filling
TMP = (64, 8.0, 2, 24)           # alpha, delta_px, persist, luma_delta: the guide is read
SRC = (128, 80)                  # the rectifier's source size
_cases = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _maps(n, w, h, seed):
    """Two int32 maps around one smooth surface, about a quarter of the pixels <= 0 (zeros and a few negatives), and the
    corner values — built as tests/test_gpu_lrcheck.py builds its own."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(1.0, DMAX / 2, (n, h, 1)) + np.cumsum(rng.normal(0, 0.4, (n, h, w)), -1)
    out = []
    for _ in range(2):
        m = np.rint(np.clip(base + rng.normal(0, 0.5, base.shape), 0.01, None) / S).astype(np.int32)
        m[rng.random(m.shape) < 0.22] = 0
        m[rng.random(m.shape) < 0.03] = -7
        out.append(m)
    l, r = out
    l[0, 0, :4] = [-7, 0, 1, 2 ** 31 - 1]
    l[-1, -1, -3:] = [-7, 2 ** 31 - 1, 1]
    r[0, 0, :3] = [2 ** 31 - 1, -7, 1]
    r[-1, -1, -2:] = [0, 1]
    return l, r


def _depth(raw, out_scale):
    """Parse's float / double mix, as tests/test_gpu_parity.py writes it -> (depth, disparity)"""
    f, B = np.float32(527.1931762695312), np.float32(119.89382172)
    dis = raw.astype(np.float32) * np.float32(out_scale)
    with np.errstate(divide="ignore"):
        depth = (np.float64(f * B) / (dis.astype(np.float64) * 16.0 * 12.0) / 1000.0).astype(np.float32)
    return depth, dis * np.float32(16.0) * np.float32(12.0)


def _case(w, h, out_scale):
    """Inputs and the twins' answers for one shape, computed once and shared by the tests (nothing here is written to)."""
    if (w, h) in _cases:
        return _cases[(w, h)]
    rng = np.random.default_rng(w * 7 + h)
    l, r = _maps(3, w, h, w + h)
    conf = rng.random(l.shape, dtype=np.float32)
    conf[0, 0, :2] = [0.5, np.nan]
    disp0 = rng.integers(0, 2 ** 32, l.shape, dtype=np.uint32).view(np.float32)
    x = rng.integers(-128, 128, (3, 6, h, w), dtype=np.int8)
    cam = pointcloud.Camera()
    # the guide: 3 NV12 frames whose pitch is not the width, noise in the chroma rows and beside the luma
    pitch = w + (w & 1) + 2
    nv = rng.integers(0, 256, (3, h + (h + 1) // 2, pitch), dtype=np.uint8)
    luma = smooth.luma_from_nv12(nv, w, h, pitch, 3)
    states = {}                      # the temporal twin's streams, carried from the first push to the second
    c = {"l": l, "r": r, "conf": conf, "disp0": disp0, "x": x, "cam": cam, "nv": nv, "pitch": pitch,
         "sm3": smooth.reference(l, luma, *SMO, out_scale=out_scale),
         "sm1": smooth.reference(r[:1], None, 1, 0, 0, out_scale=out_scale),
         "dep3": _depth(l, out_scale),
         "dep1": _depth(r[1:2], out_scale),
         "tmp3": temporal.reference(l, luma, TMP, [0, 1, 0], states, out_scale),
         "tmp1": temporal.reference(r[:1], luma[:1], TMP, [0], states, out_scale),
         "lrc1": lrcheck.reference(l[:1], r[:1], 1.0, 0.0, False, out_scale),
         "lrc3": lrcheck.reference(l, r, 0.5, 0.02, False, out_scale),
         "conf3": confidence.mask(l, conf, 0.5),
         "conf1": confidence.mask(r[2:], conf[2:], 0.25),
         "flt3": dispfilter.reference(l, *FLT, out_scale=out_scale),
         "pc2": pointcloud.reference(r[:2], cam, pointcloud.COMPACT, None, 0, out_scale),
         "pc3": pointcloud.reference(l, cam, pointcloud.ORGANISED, None, 0, out_scale),
         "mir3": lrcheck.mirror_pair(x),
         "mir1": lrcheck.mirror_pair(x[1:2])}
    if w % 4 == 0 and h % 2 == 0:      # what the rectifier asks of the model's size
        sw, sh = SRC
        calib = rectify.synthetic_rig(sw, sh, w, h, sw + w)
        eyes = rng.integers(0, 256, (2, 2, sh + sh // 2, sw), dtype=np.uint8)        # [eye][pair]
        sbs = rng.integers(0, 256, (sh + sh // 2, 2 * sw), dtype=np.uint8)           # one side-by-side frame
        rect2 = rectify.reference(calib, w, h, eyes[0], eyes[1], n=2)
        c.update(calib=calib, eyes=eyes, sbs=sbs, rect2=rect2, rect2t=rectify.tensor_from_sbs(rect2),
                 rect1=rectify.reference(calib, w, h, sbs))
    for a in c.values():
        for b in (a if isinstance(a, tuple) else (a,)):
            if isinstance(b, np.ndarray):
                b.setflags(write=False)
    _cases[(w, h)] = c
    return c


def _same3(got, want, tag):
    """(map, mask, per-map counter) of a call against the twin's"""
    for g, t, what in zip(got, want, ("map", "mask", "counter")):
        assert g.dtype == t.dtype and g.shape == t.shape and np.array_equal(g, t), f"{tag}: {what}"


def _steps(c):
    """The host-mode calls, in the order that grows and shrinks every lane's buffers beside the others': each runs on `eng`
    and compares with the twin.  The temporal filter and the rectifier are opened on `eng` by their first step and closed by
    their second."""
    l, r, conf, disp0, x, cam, nv, pitch = (c[k] for k in ("l", "r", "conf", "disp0", "x", "cam", "nv", "pitch"))
    live = {}

    def lr_check_1(eng):
        _same3(eng.lr_check(l[:1], r[:1]), c["lrc1"], "lr_check n=1")

    def conf_mask_3(eng):
        _same3(eng.conf_mask(l, conf, 0.5), c["conf3"], "conf_mask n=3")

    def filter_raw_3(eng):
        disp = disp0.copy()
        _same3(eng.filter_raw(l, *FLT, disp=disp), c["flt3"], "filter_raw n=3")
        out, mask, _ = c["flt3"]
        val = np.where(out > 0, out.astype(np.float32) * S32, np.float32(0))
        assert np.array_equal(_bits(disp), np.where(mask != 0, _bits(val), _bits(disp0))), "filter_raw n=3: disp"

    def lr_check_3(eng):
        disp = disp0.copy()
        _same3(eng.lr_check(l, r, 0.5, 0.02, False, disp), c["lrc3"], "lr_check n=3")
        assert np.array_equal(_bits(disp), np.where(c["lrc3"][1] != 0, np.uint32(0), _bits(disp0))), "lr_check n=3: disp"

    def pointcloud_compact_2(eng):
        got, gc = eng.pointcloud(r[:2], cam, pointcloud.COMPACT)
        want, wc = c["pc2"]
        assert np.array_equal(gc, wc), "pointcloud COMPACT n=2: counts"
        for k, cnt in enumerate(wc):
            assert np.array_equal(_bits(got[k, :cnt]), _bits(want[k, :cnt])), f"pointcloud COMPACT n=2: map {k}"

    def pointcloud_organised_3(eng):
        got, gc = eng.pointcloud(l, cam, pointcloud.ORGANISED)
        assert np.array_equal(gc, c["pc3"][1]) and np.array_equal(_bits(got), _bits(c["pc3"][0])), "pointcloud ORGANISED n=3"

    def conf_mask_1(eng):
        _same3(eng.conf_mask(r[2:], conf[2:], 0.25), c["conf1"], "conf_mask n=1")

    def mirror_pair_3(eng):
        assert np.array_equal(eng.mirror_pair(x), c["mir3"]), "mirror_pair n=3"

    def mirror_pair_1(eng):
        assert np.array_equal(eng.mirror_pair(x[1:2]), c["mir1"]), "mirror_pair n=1"

    def smooth_raw_3(eng):
        disp = disp0.copy()
        _same3(eng.smooth_raw(l, nv, api.SN_GUIDE_NV12, pitch, *SMO, disp=disp), c["sm3"], "smooth_raw n=3")
        out, mask, _ = c["sm3"]
        assert np.array_equal(_bits(disp), _bits(smooth.expected_disp(disp0, out, mask, eng.out_scale))), "smooth_raw n=3: disp"

    def smooth_raw_1(eng):
        _same3(eng.smooth_raw(r[:1], None, radius=1, sigma_luma=0), c["sm1"], "smooth_raw n=1")

    def depth_from_raw_3(eng):
        depth, disp = eng.depth_from_raw(l, want_disp=True)
        assert np.array_equal(_bits(depth), _bits(c["dep3"][0])) and np.array_equal(_bits(disp), _bits(c["dep3"][1])), \
            "depth_from_raw n=3"

    def depth_from_raw_1(eng):
        assert np.array_equal(_bits(eng.depth_from_raw(r[1:2])), _bits(c["dep1"][0])), "depth_from_raw n=1"

    def temporal_push_3(eng):
        live["tf"] = eng.temporal_filter(2, *TMP)
        disp = disp0.copy()
        _same3(live["tf"].push(l, nv, api.SN_GUIDE_NV12, pitch, [0, 1, 0], disp), c["tmp3"], "temporal push n=3")
        assert np.array_equal(_bits(disp), _bits(temporal.expected_disp(disp0, l, c["tmp3"][0], eng.out_scale))), \
            "temporal push n=3: disp"

    def temporal_push_1(eng):
        with live.pop("tf") as tf:
            _same3(tf.push(r[:1], nv[:1], api.SN_GUIDE_NV12, pitch), c["tmp1"], "temporal push n=1")

    def rectify_2(eng):
        live["rect"] = eng.rectifier(c["calib"])
        sbs, ten = live["rect"].rectify(c["eyes"][0], c["eyes"][1], n=2, want_tensor=True)
        assert np.array_equal(sbs, c["rect2"]) and np.array_equal(ten, c["rect2t"]), "rectify n=2"

    def rectify_1(eng):
        with live.pop("rect") as rect:
            assert np.array_equal(rect.rectify(c["sbs"]), c["rect1"]), "rectify n=1"

    steps = [lr_check_1, conf_mask_3, filter_raw_3, lr_check_3, smooth_raw_3, temporal_push_3, pointcloud_compact_2,
             depth_from_raw_3, rectify_2, pointcloud_organised_3, smooth_raw_1, conf_mask_1, temporal_push_1, depth_from_raw_1,
             mirror_pair_3, rectify_1, mirror_pair_1]
    return [s for s in steps if "calib" in c or s not in (rectify_2, rectify_1)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SHAPES)
def test_host_mode_sequence_on_one_handle(model_factory, w, h):
    with api.StereoNetHIP(model_factory(w, h, DMAX), max_batch=3) as eng:
        c = _case(w, h, eng.out_scale)
        assert 0.2 < float((c["l"] <= 0).mean()) < 0.3
        for step in _steps(c):
            step(eng)
        for step in _steps(c)[:4]:        # and once more from the top: the buffers have their final sizes now
            step(eng)


def _equal(got, want, tag):
    assert len(got) == len(want), tag
    for k, (g, t) in enumerate(zip(got, want)):
        assert g.dtype == t.dtype and g.shape == t.shape, f"{tag}: output {k}"
        assert np.array_equal(_bits(g) if g.dtype == np.float32 else g, _bits(t) if t.dtype == np.float32 else t), f"{tag}: output {k}"


@pytest.mark.gpu
def test_inference_interleaved_with_the_stateless_calls(model_factory):
    w, h = SHAPES[0]
    model = model_factory(w, h, DMAX)
    x = np.stack([synth.model_input_i8(w, h, DMAX, 80 + k) for k in range(3)])
    with api.StereoNetHIP(model, max_batch=3, precision=api.PREC_F16) as eng:
        steps = _steps(_case(w, h, eng.out_scale))
        got = [eng.infer_conf(x[:1], 0.5)]
        for step in steps[:3]:
            step(eng)
        got.append(eng.infer_lrc(x, want_right=True))
        for step in steps[3:6]:
            step(eng)
        got.append(eng.infer_conf(x, 0.5))
        for step in steps[6:]:
            step(eng)
    with api.StereoNetHIP(model, max_batch=3, precision=api.PREC_F16) as fresh:
        want = [fresh.infer_conf(x[:1], 0.5), fresh.infer_lrc(x, want_right=True), fresh.infer_conf(x, 0.5)]
    for g, t, tag in zip(got, want, ("infer_conf n=1", "infer_lrc n=3", "infer_conf n=3")):
        _equal(g, t, tag)
    assert int(got[1][3].min()) > 0 and int(got[2][4].min()) > 0        # kept pixels per map: the maps are not trivially empty


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SHAPES)
def test_device_mode_then_host_mode(model_factory, w, h):
    """A device-mode call on a caller stream touches no staging buffer; the host-mode call of the same entry point after it
    stages everything for the first time."""
    import torch
    with api.StereoNetHIP(model_factory(w, h, DMAX), max_batch=3) as eng:
        c = _case(w, h, eng.out_scale)
        l, r, disp0 = c["l"], c["r"], c["disp0"]
        s1 = torch.cuda.Stream()

        def dev(a):
            return torch.from_numpy(a.copy()).cuda()

        # lr_check: masked in place, float map, mask and kept
        t_l, t_r, t_disp = dev(l), dev(r), dev(disp0)
        t_mask = torch.zeros(l.shape, dtype=torch.uint8, device="cuda")
        t_kept = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        eng.lr_check_device(3, t_l.data_ptr(), t_r.data_ptr(), 0.5, 0.02, False, t_l.data_ptr(), t_disp.data_ptr(),
                            t_mask.data_ptr(), t_kept.data_ptr(), stream=s1.cuda_stream)
        s1.synchronize()
        want = c["lrc3"]
        _same3((t_l.cpu().numpy(), t_mask.cpu().numpy(), t_kept.cpu().numpy().view(np.uint32)), want, "lr_check device")
        assert np.array_equal(_bits(t_disp.cpu().numpy()), np.where(want[1] != 0, np.uint32(0), _bits(disp0)))
        assert np.array_equal(t_r.cpu().numpy(), r)
        disp = disp0.copy()
        _same3(eng.lr_check(l, r, 0.5, 0.02, False, disp), want, "lr_check host")
        assert np.array_equal(_bits(disp), np.where(want[1] != 0, np.uint32(0), _bits(disp0)))

        # filter_raw: into a second map, float map, mask and counts
        t_raw, t_disp = dev(l), dev(disp0)
        t_out = torch.zeros_like(t_raw)
        t_mask.zero_()
        t_counts = torch.full((3, 3), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        eng.filter_raw_device(3, t_raw.data_ptr(), *FLT, out_raw_ptr=t_out.data_ptr(), mask_ptr=t_mask.data_ptr(),
                              disp_ptr=t_disp.data_ptr(), counts_ptr=t_counts.data_ptr(), stream=s1.cuda_stream)
        s1.synchronize()
        want = c["flt3"]
        val = np.where(want[0] > 0, want[0].astype(np.float32) * S32, np.float32(0))
        want_disp = np.where(want[1] != 0, _bits(val), _bits(disp0))
        _same3((t_out.cpu().numpy(), t_mask.cpu().numpy(), t_counts.cpu().numpy().view(np.uint32)), want, "filter_raw device")
        assert np.array_equal(_bits(t_disp.cpu().numpy()), want_disp) and np.array_equal(t_raw.cpu().numpy(), l)
        disp = disp0.copy()
        _same3(eng.filter_raw(l, *FLT, disp=disp), want, "filter_raw host")
        assert np.array_equal(_bits(disp), want_disp)
