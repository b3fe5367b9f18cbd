"""The host staging the post-processing entry points share (csrc/sn_postproc.hpp) on the MI355X: ONE handle's grow-only
buffers used by different entry points in growing and shrinking order, inference interleaved with the stateless calls, and
device mode followed by host mode.  Every result equals its numpy twin (or a fresh handle's result) bit for bit: a stale
capacity, a slot shared by two meanings or a download of the previous call's size would show up as a wrong map.
96x64 takes the vector paths, 33x47 (W % 4 != 0, odd height) the scalar ones."""
import numpy as np
import pytest

from hobot_stereonet_amd import api, confidence, dispfilter, lrcheck, pointcloud, synth

SHAPES = [(96, 64), (33, 47)]
DMAX = 48
S = float(lrcheck.wire_scale())
S32 = dispfilter.wire_scale()
FLT = (6, 1.0, 16)               # speckle_max_px, speckle_diff_px, fill_max_px: both passes of the filter
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
    c = {"l": l, "r": r, "conf": conf, "disp0": disp0, "x": x, "cam": cam,
         "lrc1": lrcheck.reference(l[:1], r[:1], 1.0, 0.0, False, out_scale),
         "lrc3": lrcheck.reference(l, r, 0.5, 0.02, False, out_scale),
         "conf3": confidence.mask(l, conf, 0.5),
         "conf1": confidence.mask(r[2:], conf[2:], 0.25),
         "flt3": dispfilter.reference(l, *FLT, out_scale=out_scale),
         "pc2": pointcloud.reference(r[:2], cam, pointcloud.COMPACT, None, 0, out_scale),
         "pc3": pointcloud.reference(l, cam, pointcloud.ORGANISED, None, 0, out_scale),
         "mir3": lrcheck.mirror_pair(x),
         "mir1": lrcheck.mirror_pair(x[1:2])}
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
    """The stateless host-mode calls, in the order that grows and shrinks the shared buffers: each runs on `eng` and compares
    with the twin."""
    l, r, conf, disp0, x, cam = (c[k] for k in ("l", "r", "conf", "disp0", "x", "cam"))

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

    return [lr_check_1, conf_mask_3, filter_raw_3, lr_check_3, pointcloud_compact_2, pointcloud_organised_3, conf_mask_1,
            mirror_pair_3, mirror_pair_1]


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
