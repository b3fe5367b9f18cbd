"""sn_infer_conf / sn_conf_mask on the MI355X: the confidence plane of the soft-argmin epilogue and its x16 upsample against the
numpy twin (hobot_stereonet_amd/confidence.py) on the kernel's own cost, against the float64 truth the project's way, the mask
as the contract on the kernel's own numbers, the plumbing (piped schedule, NV12, device mode, SN_PREC_AUTO's repeat, the call
count), argument errors and the file-list harness's --conf.

Bounds.  conf_low against confidence.low(cost, disp_low) of the SAME call (the bracket k comes from the kernel's own
disp_low, so there is no floor boundary and no pixel is left out): expf within 1 ulp, one rounded subtraction per argument, at
most 16 terms in se, one division — about (Dl + 3) * 2^-23 = 2.3e-6 for 16 planes; the bound is 1e-5.  out_conf against
confidence.upsample(conf_low): the x16 weights are exact in fp32, the values at most 1, three roundings: 1e-6.
Against the truth (160x96 D=96, gain 1, seeds 4 and 5; the truth's dhat stays 1.9e-3 and 2.4e-3 planes away from an integer
there, so no pixel is left out either): mean and max of |conf_low - twin(truth)| at most truth_compare.FP32_FACTOR (SN_PREC_FP32)
/ X3_FACTOR (SN_PREC_F16X3) times what the CPU fp32 oracle's own cost and disp_low give through the same twin."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import truth_compare as tc
from hobot_stereonet_amd import api, confidence, synth, weights

pytestmark = pytest.mark.gpu

SEEDS = (4, 5)
# (w, h, D, gain of agg.out)
POINTS = [(160, 96, 96, 1.0), (160, 96, 96, 4.0), (160, 96, 96, 16.0), (96, 64, 256, 4.0), (33, 47, 64, 4.0), (96, 64, 16, 4.0),
          (16, 16, 256, 4.0)]
LOW_TOL, UP_TOL = 1e-5, 1e-6
_blobs, _models = {}, {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _blob(gain):
    if gain not in _blobs:
        _blobs[gain] = tc.scaled(weights.synthetic(0), "agg.out", gain, 1)
    return _blobs[gain]


@pytest.fixture(scope="module")
def scaled_model(tmp_path_factory):
    """-> f(w, h, d, gain) -> path of a model file whose agg.out layer is scaled by `gain` (how sharp the soft-argmin is)"""
    def make(w, h, d, gain):
        key = (w, h, d, gain)
        if key not in _models:
            p = str(tmp_path_factory.mktemp("conf") / f"sn_{w}x{h}_d{d}_g{gain:g}.snw")
            weights.save_snw(p, _blob(gain), w, h, d)
            _models[key] = p
        return _models[key]
    return make


def _x(w, h, d, seed):
    return synth.model_input_i8(w, h, d, seed)


def _low_stages(eng, d):
    hl, wl = (eng.height + 15) // 16, (eng.width + 15) // 16
    return (eng.dbg_read("cost").reshape(d // 16, hl, wl).copy(), eng.dbg_read("disp_low").reshape(hl, wl).copy(),
            eng.dbg_read("conf_low").reshape(hl, wl).copy())


# ---- 1. the kernels against the twin -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,d,gain", POINTS, ids=[f"{w}x{h}-d{d}-g{g:g}" for w, h, d, g in POINTS])
def test_kernels_against_the_twin(scaled_model, w, h, d, gain):
    path = scaled_model(w, h, d, gain)
    modes = [api.PREC_F16, api.PREC_F16X3] + ([api.PREC_FP32] if (w, h, d, gain) == (160, 96, 96, 4.0) else [])
    got = {}
    for prec in modes:
        with api.StereoNetHIP(path, precision=prec) as eng:
            for seed in SEEDS:
                disp, raw, conf = eng.infer_conf(_x(w, h, d, seed))
                cost, disp_low, conf_low = _low_stages(eng, d)
                tag = f"{api.PREC_NAMES[prec]} seed {seed}"
                assert conf.shape == (h, w) and np.isfinite(conf_low).all() and np.isfinite(conf).all(), tag
                e_low = np.abs(conf_low.astype(np.float64) - confidence.low(cost, disp_low))
                e_up = np.abs(conf.astype(np.float64) - confidence.upsample(conf_low, h, w))
                print(f"{w}x{h} D={d} gain {gain:g} {tag}: conf_low {conf_low.min():.3f}..{conf_low.max():.3f} median "
                      f"{np.median(conf_low):.3f} share >= 0.5 {(conf_low >= 0.5).mean():.2f}; |conf_low - twin| max {e_low.max():.2e}, "
                      f"|out_conf - upsample| max {e_up.max():.2e}")
                assert e_low.max() <= LOW_TOL, tag                       # every pixel
                assert e_up.max() <= UP_TOL, tag
                assert conf_low.min() >= 0.0 and conf_low.max() <= 1.0 + LOW_TOL, tag
                if d == 16:                                               # one plane: 1.0f, and the exact weights keep it
                    assert np.all(_bits(conf_low) == _bits(np.float32(1.0))) and np.all(_bits(conf) == _bits(np.float32(1.0))), tag
                got[(prec, seed)] = (conf_low, conf, disp, raw)
    for seed in SEEDS:                                                    # the low-resolution branch takes no mode
        a, b = got[(api.PREC_F16, seed)], got[(api.PREC_F16X3, seed)]
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])), f"seed {seed}"
    if d > 16 and (w, h) != (16, 16):                                    # not a constant plane
        assert np.ptp(got[(api.PREC_F16, SEEDS[0])][0]) > 0.05


# ---- 2. against the truth ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_conf_low_against_the_truth(oracle, scaled_model, seed):
    import torch_ref
    w, h, d, gain = 160, 96, 96, 1.0
    blob, x = _blob(gain), _x(w, h, d, seed)
    truth = torch_ref.truth(blob, x, d)
    t_low = np.asarray(truth["disp_low"], np.float64)
    print(f"\nseed {seed}: the truth's dhat stays {np.abs(t_low - np.rint(t_low)).min():.2e} planes away from an integer")
    want = confidence.low(truth["cost"], t_low.astype(np.float32))
    fl = oracle.features(blob, x[:3].astype(np.float32) / 128.0)
    fr = oracle.features(blob, x[3:].astype(np.float32) / 128.0)
    o_cost = oracle.aggregate(blob, fl, fr, d // 16)
    o_err = np.abs(confidence.low(o_cost, oracle.soft_argmin(o_cost)) - want)
    e_ref, m_ref = float(o_err.mean()), float(o_err.max())
    print(f"   CPU fp32 oracle through the twin: E_ref {e_ref:.3e} M_ref {m_ref:.3e}")
    bad = []
    for name, prec, factor in (("fp32", api.PREC_FP32, tc.FP32_FACTOR), ("f16x3", api.PREC_F16X3, tc.X3_FACTOR)):
        with api.StereoNetHIP(scaled_model(w, h, d, gain), precision=prec) as eng:
            eng.infer_conf(x)
            _, _, conf_low = _low_stages(eng, d)
        err = np.abs(conf_low.astype(np.float64) - want)                  # every pixel
        e, m = float(err.mean()), float(err.max())
        print(f"   {name:<6} E {e:.3e} ({e / e_ref:.2f} x E_ref)  M {m:.3e} ({m / m_ref:.2f} x M_ref)  bound {factor:g} x")
        if not e <= factor * e_ref:
            bad.append(f"{name}: mean {e:.3e} > {factor:g} x {e_ref:.3e}")
        if not m <= factor * m_ref:
            bad.append(f"{name}: max {m:.3e} > {factor:g} x {m_ref:.3e}")
    assert not bad, "\n".join(bad)


# ---- 3. the mask is the contract on the kernel's own numbers -----------------------------------------------------------------
@pytest.mark.parametrize("w,h,d,gain", [(160, 96, 96, 4.0), (33, 47, 64, 4.0)], ids=["160x96", "33x47"])
def test_mask_is_the_contract(scaled_model, w, h, d, gain):
    import torch
    x = np.stack([_x(w, h, d, s) for s in SEEDS])
    with api.StereoNetHIP(scaled_model(w, h, d, gain), max_batch=2, precision=api.PREC_F16) as eng:
        disp_plain, raw_plain = eng.infer(x)
        disp0, raw0, conf = eng.infer_conf(x)                             # p = NULL: the plain map plus the confidence
        assert np.array_equal(raw0, raw_plain) and np.array_equal(_bits(disp0), _bits(disp_plain))
        print(f"\n{w}x{h}: {int(((raw_plain == 0) & (disp_plain != 0)).sum())} pixels with raw == 0 and a non-zero float disparity")
        for min_conf in (0.0, 0.5, 0.7, 1.0):
            disp, raw, cf, mask, kept = eng.infer_conf(x, min_conf)
            tag = f"min_conf {min_conf}"
            assert np.array_equal(_bits(cf), _bits(conf)), tag
            want_mask = np.where(raw_plain <= 0, 1, np.where(conf >= np.float32(min_conf), 0, 64)).astype(np.uint8)
            assert np.array_equal(mask, want_mask), tag
            assert np.array_equal(raw, np.where(mask == 0, raw_plain, 0)), tag
            assert np.array_equal(_bits(disp), np.where(mask != 0, np.uint32(0), _bits(disp_plain))), tag
            assert kept.dtype == np.uint32 and np.array_equal(kept, (mask == 0).reshape(2, -1).sum(1)), tag
            t_out, t_mask, t_kept = confidence.mask(raw_plain, conf, min_conf)      # and the twin says the same
            assert np.array_equal(t_out, raw) and np.array_equal(t_mask, mask) and np.array_equal(t_kept, kept), tag
            share = float((mask == 0).mean())
            print(f"   {tag}: kept {kept.tolist()} of {w * h} ({share:.3f})")
            if min_conf == 0.0:                                           # nothing is rejected for its confidence
                assert not (mask == 64).any()
                assert np.array_equal(raw, raw_plain) and np.array_equal(_bits(disp), _bits(disp_plain))
            if min_conf == 0.5 and (w, h) == (160, 96):                   # both outcomes occur: no constant plane passes
                assert 0.2 < share < 0.98
            # the stateless call on the same raw and confidence: host buffers, then device pointers in place
            d2 = disp_plain.copy()
            o2, m2, k2 = eng.conf_mask(raw_plain, conf, min_conf, d2)
            assert np.array_equal(o2, raw) and np.array_equal(m2, mask) and np.array_equal(k2, kept), tag
            assert np.array_equal(_bits(d2), _bits(disp)), tag
            t_raw, t_conf, t_disp = (torch.from_numpy(a.copy()).cuda() for a in (raw_plain, conf, disp_plain))
            t_m = torch.zeros(mask.shape, dtype=torch.uint8, device="cuda")
            t_k = torch.full((2,), 7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            eng.conf_mask_device(2, t_raw.data_ptr(), t_conf.data_ptr(), min_conf, out_raw_ptr=t_raw.data_ptr(),
                                 disp_ptr=t_disp.data_ptr(), mask_ptr=t_m.data_ptr(), kept_ptr=t_k.data_ptr())
            assert np.array_equal(t_raw.cpu().numpy(), raw) and np.array_equal(t_m.cpu().numpy(), mask), tag
            assert np.array_equal(_bits(t_disp.cpu().numpy()), _bits(disp)), tag
            assert np.array_equal(t_k.cpu().numpy().view(np.uint32), kept), tag
        # a single pair drops the leading dimension and equals the first pair of the batch; the float map alone
        d1, r1, c1, m1, k1 = eng.infer_conf(x[0], 0.5)
        _, r2, _, m2, k2 = eng.infer_conf(x, 0.5)
        assert r1.shape == (h, w) and np.array_equal(r1, r2[0]) and np.array_equal(m1, m2[0]) and k1.tolist() == k2[:1].tolist()
        # a NaN confidence is rejected at every threshold, 0 included
        cn = conf.copy()
        cn[0, 0, :3] = np.nan
        _, mn, _ = eng.conf_mask(np.maximum(raw_plain, 1), cn, 0.0)
        assert mn[0, 0, :3].tolist() == [64, 64, 64] and int((mn != 0).sum()) == 3


# ---- 4. plumbing -------------------------------------------------------------------------------------------------------------
def test_piped_batch_equals_single_calls(scaled_model):
    w, h, d = 160, 96, 96
    x = np.stack([_x(w, h, d, 10 + k) for k in range(5)])
    path = scaled_model(w, h, d, 4.0)
    # refine_chunk = 1: at this size the library would take the whole batch as one tower chunk, and a piece is never smaller
    # than a chunk — the call would then be one piece on the plain schedule
    with api.StereoNetHIP(path, max_batch=5, piece=2, refine_chunk=1, precision=api.PREC_F16) as eng:
        assert eng.piece == 2 and eng.refine_chunk == 1                   # three pieces, n > chunk: the piped schedule
        before = eng.infer(x)
        calls0 = eng.refine_stats()["calls"]
        batch = eng.infer_conf(x, 0.5)
        assert eng.refine_stats()["calls"] == calls0 + 1                  # one forward
        plain = eng.infer_conf(x)
        assert eng.refine_stats()["calls"] == calls0 + 2
        singles = [eng.infer_conf(x[k], 0.5) for k in range(5)]
        assert eng.refine_stats()["calls"] == calls0 + 7
        after = eng.infer(x)
    for k in range(5):                                                    # piece-indexed conf_low, every piece of the pipe
        for i in range(4):
            assert np.array_equal(_bits(batch[i][k]), _bits(singles[k][i])), (k, i)
        assert singles[k][4].tolist() == batch[4][k:k + 1].tolist()
        assert np.array_equal(_bits(plain[2][k]), _bits(singles[k][2]))
    assert len({batch[2][k].tobytes() for k in range(5)}) == 5            # five different planes
    assert np.array_equal(after[1], before[1]) and np.array_equal(_bits(after[0]), _bits(before[0]))
    assert np.array_equal(plain[1], before[1]) and np.array_equal(_bits(plain[0]), _bits(before[0]))


def test_nv12_input_and_device_mode(scaled_model):
    import torch
    w, h, d, n = 160, 96, 96, 2
    frames = np.stack([synth.sbs_nv12_frame(w, h, d, 20 + k) for k in range(n)])
    with api.StereoNetHIP(scaled_model(w, h, d, 4.0), max_batch=n, precision=api.PREC_F16) as eng:
        x = eng.preprocess_sbs_nv12(frames)
        want = eng.infer_conf(x, 0.5)
        got = eng.infer_conf(frames, 0.5)
        for g, t in zip(got, want):
            assert np.array_equal(_bits(g) if g.dtype == np.float32 else g, _bits(t) if t.dtype == np.float32 else t)
        one = eng.infer_conf(frames[0], 0.5)                              # one flat frame
        assert one[1].shape == (h, w) and np.array_equal(one[1], want[1][0])
        disp, raw, conf, mask, kept = want
        # device pointers on a caller stream
        dx = torch.from_numpy(x).cuda()
        t_raw = torch.empty((n, h, w), dtype=torch.int32, device="cuda")
        t_disp = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
        t_conf = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
        t_mask = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
        t_kept = torch.empty(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s1 = torch.cuda.Stream()
        eng.infer_conf_device(n, dx.data_ptr(), 0.5, t_raw.data_ptr(), t_disp.data_ptr(), t_conf.data_ptr(), t_mask.data_ptr(),
                              t_kept.data_ptr(), stream=s1.cuda_stream)
        s1.synchronize()
        assert np.array_equal(t_raw.cpu().numpy(), raw) and np.array_equal(t_mask.cpu().numpy(), mask)
        assert np.array_equal(_bits(t_disp.cpu().numpy()), _bits(disp)) and np.array_equal(_bits(t_conf.cpu().numpy()), _bits(conf))
        assert np.array_equal(t_kept.cpu().numpy().view(np.uint32), kept)
        # the float map alone (the rules read a map of the engine's own), device NV12 frames, the engine's stream
        t_disp.fill_(-1.0)
        t_mask.fill_(9)
        df = torch.from_numpy(frames).cuda()
        torch.cuda.synchronize()
        eng.infer_conf_device(n, df.data_ptr(), 0.5, disp_ptr=t_disp.data_ptr(), mask_ptr=t_mask.data_ptr(),
                              in_kind=api.SN_LRC_IN_SBS_NV12)
        assert np.array_equal(_bits(t_disp.cpu().numpy()), _bits(disp)) and np.array_equal(t_mask.cpu().numpy(), mask)
        # the stateless call on the caller's stream
        t_raw2 = torch.from_numpy(eng.infer(x)[1]).cuda()
        torch.cuda.synchronize()
        eng.conf_mask_device(n, t_raw2.data_ptr(), t_conf.data_ptr(), 0.5, mask_ptr=t_mask.data_ptr(), kept_ptr=t_kept.data_ptr(),
                             stream=s1.cuda_stream)
        s1.synchronize()
        assert np.array_equal(t_mask.cpu().numpy(), mask) and np.array_equal(t_kept.cpu().numpy().view(np.uint32), kept)


def test_default_precision_repeat_masks_the_repeated_maps(tmp_path):
    """S-noise-g8: the first call of a fresh default-precision handle leaves the fp16 tower's envelope and is repeated in
    SN_PREC_F16X3; every output then belongs to that arithmetic."""
    w, h, d, levels, wk, kind = tc.DOMAIN["S-noise-g8"]
    path = str(tmp_path / "m.snw")
    weights.save_snw(path, tc.domain_blob(levels, wk), w, h, d)
    x = tc.domain_input(w, h, d, kind)
    with api.StereoNetHIP(path, precision=api.PREC_F16X3) as eng:
        want = eng.infer_conf(x, 0.5)
        want_low = eng.dbg_read("conf_low").copy()
    with api.StereoNetHIP(path, precision=api.PREC_DEFAULT) as eng:
        st0 = eng.refine_stats()
        got = eng.infer_conf(x, 0.5)
        st1 = eng.refine_stats()
        got_low = eng.dbg_read("conf_low").copy()
    assert st1["reruns"] == st0["reruns"] + 1 and st1["calls"] == st0["calls"] + 1 and st1["precision_last"] == "f16x3"
    for g, t in zip(got, want):
        assert np.array_equal(_bits(g) if g.dtype == np.float32 else g, _bits(t) if t.dtype == np.float32 else t)
    assert np.array_equal(_bits(got_low), _bits(want_low))
    print(f"\nS-noise-g8: kept {got[4].tolist()} of {w * h}")


# ---- 5. argument errors --------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_handle_usable(model_factory):
    w, h, d = 96, 64, 48
    x = np.stack([_x(w, h, d, 60 + k) for k in range(2)])
    with api.StereoNetHIP(model_factory(w, h, d), max_batch=2, precision=api.PREC_F16) as eng:
        before = eng.infer(x)
        lib, hd = eng._lib, eng._h
        r = np.ones((2, h, w), np.int32)
        c = np.ones((2, h, w), np.float32)
        o = np.empty_like(r)
        dsp = np.empty((2, h, w), np.float32)
        msk = np.empty((2, h, w), np.uint8)
        kpt = np.zeros(2, np.uint32)
        frames = np.zeros(2 * 3 * h * w, np.uint8)
        ok = api.SnConfParams(0.5)
        P = C.byref

        def inf(n=1, inp=x, kind=0, p=ok, out=o, disp=None, conf=None, mask=None, kept=None, w2=2 * w, hp=h):
            return lib.sn_infer_conf(hd, n, api._np_ptr(inp), kind, w2, hp, P(p) if p is not None else None, api._np_ptr(out),
                                     api._np_ptr(disp), api._np_ptr(conf), api._np_ptr(mask), api._np_ptr(kept), api.SN_MEM_HOST, None)

        def cm(n=1, raw=r, conf=c, p=ok, out=o, disp=None, mask=None, kept=None):
            return lib.sn_conf_mask(hd, n, api._np_ptr(raw), api._np_ptr(conf), P(p) if p is not None else None, api._np_ptr(out),
                                    api._np_ptr(disp), api._np_ptr(mask), api._np_ptr(kept), api.SN_MEM_HOST, None)

        assert inf() == 0 and inf(out=None, disp=dsp) == 0 and inf(p=None, conf=c.copy()) == 0 and inf(inp=frames, kind=1) == 0
        assert inf(n=2, mask=msk, kept=kpt) == 0 and inf(p=api.SnConfParams(0.0)) == 0 and inf(p=api.SnConfParams(1.0)) == 0
        assert cm() == 0 and cm(out=None, mask=msk) == 0 and cm(n=2, disp=dsp, mask=msk, kept=kpt) == 0
        bad_p = [api.SnConfParams(-0.1), api.SnConfParams(1.5), api.SnConfParams(float("nan")), api.SnConfParams(float("inf")),
                 api.SnConfParams(float("-inf"))]
        for p in bad_p:
            assert inf(p=p) == -1 and cm(p=p) == -1
        assert cm(p=None) == -1                                           # the stateless call needs a threshold
        assert inf(p=None, mask=msk) == -1 and inf(p=None, kept=kpt) == -1      # no masking: no mask, no count
        for n in (0, -1, 3):
            assert inf(n=n) == -1 and cm(n=n) == -1
        assert inf(inp=None) == -1 and inf(out=None, disp=None) == -1
        assert inf(kind=2) == -1 and inf(kind=-1) == -1
        assert inf(inp=frames, kind=1, w2=w) == -1 and inf(inp=frames, kind=1, hp=h + 2) == -1      # geometry
        assert cm(raw=None) == -1 and cm(conf=None) == -1 and cm(out=None, mask=None) == -1
        as_i32, as_u8 = c.view(np.int32), c.view(np.uint8).reshape(-1)[:2 * h * w].reshape(2, h, w)
        assert cm(out=as_i32) == -1 and cm(disp=c) == -1 and cm(mask=as_u8) == -1      # conf aliasing an output
        assert cm(n=2, kept=c.view(np.uint32).reshape(-1)[-2:]) == -1
        assert "sn_conf_mask" in lib.sn_last_error(hd).decode()
        assert cm(out=r) == 0                                             # out_raw == raw is allowed
        with pytest.raises(api.StereoNetError):
            eng.conf_mask(r[:, :-1], c[:, :-1], 0.5)
        with pytest.raises(api.StereoNetError):
            eng.infer_conf(np.zeros(7, np.uint8))
        after = eng.infer(x)
        assert np.array_equal(after[1], before[1]) and np.array_equal(_bits(after[0]), _bits(before[0]))


# ---- 6. the file-list harness --------------------------------------------------------------------------------------------------
def test_filelist_conf(model_factory, tmp_path, capsys):
    from hobot_stereonet_amd import filelist, images, render
    w, h, d = 96, 64, 48
    model = model_factory(w, h, d)
    names = {"l": [], "r": []}
    for k in range(2):
        lt, rt = synth.stereo_pair_u8(w, h, d, 70 + k)
        for side, eye in (("l", lt), ("r", rt)):
            p = str(tmp_path / f"{side}{k}.ppm")
            images.write_ppm(p, np.ascontiguousarray(eye.transpose(1, 2, 0)))
            names[side].append(p)
    gts = []
    for k in range(2):
        p = str(tmp_path / f"gt{k}.pfm")
        images.write_pfm(p, synth.disparity_field(w, h, d))
        gts.append(p)
    for side, lst in (("l", names["l"]), ("r", names["r"]), ("gt", gts)):
        (tmp_path / f"{side}.list").write_text("".join(f"{p}\n" for p in lst))
    base = ["--model", model, "--left", str(tmp_path / "l.list"), "--right", str(tmp_path / "r.list"), "--precision", "f16"]
    capsys.readouterr()
    assert filelist.main(base + ["--out", str(tmp_path / "plain")]) == 0
    plain_summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert filelist.main(base + ["--out", str(tmp_path / "conf"), "--gt", str(tmp_path / "gt.list"), "--conf", "0.5"]) == 0
    conf_summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert filelist.main(base + ["--out", str(tmp_path / "both"), "--conf", "0.5", "--lrc", "1"]) == 0
    both_summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert plain_summary == {"frames": 2}                                      # without the flag: the summary of before
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(f"{i}.{e}" for i in (0, 1) for e in ("raw.bin", "disp.pfm", "depth.ppm"))
    with_conf = sorted(f"{i}.{e}" for i in (0, 1) for e in ("raw.bin", "disp.pfm", "depth.ppm", "mask.pgm", "conf.pfm"))
    assert sorted(os.listdir(tmp_path / "conf")) == with_conf and sorted(os.listdir(tmp_path / "both")) == with_conf
    rd = lambda p: open(p, "rb").read()      # noqa: E731
    densities, both_densities = [], []
    with api.StereoNetHIP(model, precision=api.PREC_F16) as eng:
        for i in range(2):
            eyes = [images.bgr_to_nv12(images.imread_bgr(names[s][i])) for s in ("l", "r")]
            sbs = images.sbs_from_eyes(eyes[0], eyes[1], w, h)
            # without the flag every file is what the unchanged code path writes from infer_sbs_nv12
            disp, raw = eng.infer_sbs_nv12(sbs)
            images.write_pfm(str(tmp_path / "want.pfm"), disp)
            _, depth = render.disparity_and_depth(raw.view(np.uint32))
            images.write_ppm(str(tmp_path / "want.ppm"), render.colorize_depth(depth)[..., ::-1])
            assert rd(tmp_path / "plain" / f"{i}.raw.bin") == raw.tobytes()
            assert rd(tmp_path / "plain" / f"{i}.disp.pfm") == rd(tmp_path / "want.pfm")
            assert rd(tmp_path / "plain" / f"{i}.depth.ppm") == rd(tmp_path / "want.ppm")
            # with it: byte for byte the results of infer_conf
            mdisp, mraw, conf, mask, kept = eng.infer_conf(sbs, 0.5)
            for name, arr in (("want.pfm", mdisp), ("wantc.pfm", conf)):
                images.write_pfm(str(tmp_path / name), arr)
            images.write_ppm(str(tmp_path / "want.pgm"), mask)
            _, depth = render.disparity_and_depth(mraw.view(np.uint32))
            images.write_ppm(str(tmp_path / "want.ppm"), render.colorize_depth(depth)[..., ::-1])
            assert rd(tmp_path / "conf" / f"{i}.raw.bin") == mraw.tobytes()
            assert rd(tmp_path / "conf" / f"{i}.disp.pfm") == rd(tmp_path / "want.pfm")
            assert rd(tmp_path / "conf" / f"{i}.conf.pfm") == rd(tmp_path / "wantc.pfm")
            assert rd(tmp_path / "conf" / f"{i}.mask.pgm") == rd(tmp_path / "want.pgm")
            assert rd(tmp_path / "conf" / f"{i}.depth.ppm") == rd(tmp_path / "want.ppm")
            assert np.array_equal(mraw, np.where(mask == 0, raw, 0))
            densities.append(float(kept[0]) / (w * h))
            # --conf with --lrc: the composition of the public calls, two forwards
            calls0 = eng.refine_stats()["calls"]
            cdisp, craw, cconf = eng.infer_conf(sbs)
            _, raw_m = eng.infer(eng.mirror_pair(eng.preprocess_sbs_nv12(sbs)[0]))
            assert eng.refine_stats()["calls"] == calls0 + 2
            cdisp = cdisp.copy()
            lraw, lmask, _ = eng.lr_check(craw, raw_m, 1.0, 0.0, True, cdisp)
            fraw, cmask, ckept = eng.conf_mask(lraw, cconf, 0.5, cdisp)
            assert rd(tmp_path / "both" / f"{i}.raw.bin") == fraw.tobytes()
            assert np.array_equal(images.read_pnm(str(tmp_path / "both" / f"{i}.mask.pgm")), lmask | cmask)
            assert np.array_equal(_bits(images.read_pfm(str(tmp_path / "both" / f"{i}.disp.pfm"))), _bits(cdisp))
            assert np.array_equal(_bits(images.read_pfm(str(tmp_path / "both" / f"{i}.conf.pfm"))), _bits(conf))
            assert np.array_equal(fraw, np.where((lmask | cmask) == 0, raw, 0))
            both_densities.append(float(ckept[0]) / (w * h))
        recs = filelist.run_imglist(eng, str(tmp_path / "l.list"), str(tmp_path / "r.list"), gt_list=str(tmp_path / "gt.list"),
                                    conf=0.5)
        gt = synth.disparity_field(w, h, d)
        for rec in recs:
            assert rec["metrics"]["valid_px"] == int(((rec["mask"] == 0) & (gt < d)).sum())      # kept and valid ground truth
    assert conf_summary["frames"] == 2 and conf_summary["density"] == pytest.approx(np.mean(densities), abs=1e-12)
    assert set(conf_summary) == {"frames", "epe", "bad1", "bad3", "d1", "density"}
    assert set(both_summary) == {"frames", "density"} and both_summary["density"] == pytest.approx(np.mean(both_densities), abs=1e-12)
