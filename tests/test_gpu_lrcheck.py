"""sn_mirror_pair_i8 / sn_lr_check / sn_infer_lrc on the MI355X: the kernels equal the numpy twin
(hobot_stereonet_amd/lrcheck.py) bit for bit, the composite equals the composition of the existing calls, the right eye's map
of a mirror-symmetric input, agreement with the point cloud, device mode on a caller stream, argument errors and the file-list
harness's --lrc."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from hobot_stereonet_amd import api, lrcheck, pointcloud, synth

SHAPES = [(96, 64), (1242, 375), (1280, 720)]
D = {(96, 64): 48, (1242, 375): 256, (1280, 720): 192}
TAUS = [(1.0, 0.0), (0.5, 0.02), (0.0, 0.0)]
S = float(lrcheck.wire_scale())


def _maps(n, w, h, dmax, seed):
    """Two int32 maps around one smooth surface (so that every reason occurs), ~30 % zeros, and the corner values."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(1.0, dmax / 2, (n, h, 1)) + np.cumsum(rng.normal(0, 0.4, (n, h, w)), -1)
    out = []
    for _ in range(2):
        m = np.rint(np.clip(base + rng.normal(0, 0.5, base.shape), 0.01, None) / S).astype(np.int32)
        m[rng.random(m.shape) < 0.3] = 0
        out.append(m)
    l, r = out
    l[0, 0, :4] = [-7, 0, 1, 2 ** 31 - 1]
    l[-1, -1, -3:] = [-7, 2 ** 31 - 1, 1]
    r[0, 0, :3] = [2 ** 31 - 1, -7, 1]
    r[-1, -1, -2:] = [0, 1]
    return l, r


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SHAPES)
def test_kernels_equal_twin_bit_for_bit(model_factory, w, h):
    import torch
    rng = np.random.default_rng(w)
    l3, r3 = _maps(3, w, h, D[(w, h)], w + h)
    x3 = rng.integers(-128, 128, (3, 6, h, w), dtype=np.int8)
    seen = set()
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=3) as eng:
        for n in (1, 3):
            got = eng.mirror_pair(x3[:n])
            assert np.array_equal(got, lrcheck.mirror_pair(x3[:n])), f"mirror n={n}"
            l, r = l3[-n:], r3[-n:]
            for mirrored in (False, True):
                rr = np.ascontiguousarray(r[..., ::-1]) if mirrored else r
                for tau_px, tau_rel in TAUS:
                    tag = f"n={n} mirrored={mirrored} tau=({tau_px}, {tau_rel})"
                    disp0 = rng.integers(0, 2 ** 32, l.shape, dtype=np.uint32).view(np.float32)
                    disp = disp0.copy()
                    out, mask, kept = eng.lr_check(l, rr, tau_px, tau_rel, mirrored, disp)
                    w_out, w_mask, w_kept = lrcheck.reference(l, rr, tau_px, tau_rel, mirrored, eng.out_scale)
                    assert np.array_equal(mask, w_mask), tag
                    assert np.array_equal(out, w_out) and np.array_equal(kept, w_kept), tag
                    assert np.array_equal(_bits(disp), np.where(w_mask != 0, np.uint32(0), _bits(disp0))), tag
                    seen |= set(np.unique(w_mask).tolist())
        assert seen == {0, 1, 2, 4, 8}                       # the maps reach every reason
        single, _, _ = eng.lr_check(l3[0], r3[0])            # a 2-D map is one map
        assert np.array_equal(single, lrcheck.reference(l3[0], r3[0], out_scale=eng.out_scale)[0])
        # device pointers, masked in place (out_raw == raw_left), mask and kept alone, and the device mirror
        want = lrcheck.reference(l3, r3, 0.5, 0.02, False, eng.out_scale)
        dl, dr = torch.from_numpy(l3).cuda(), torch.from_numpy(r3).cuda()
        dk = torch.zeros(3, dtype=torch.int32, device="cuda")
        dm = torch.zeros(l3.shape, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        eng.lr_check_device(3, dl.data_ptr(), dr.data_ptr(), 0.5, 0.02, False, mask_ptr=dm.data_ptr(), kept_ptr=dk.data_ptr())
        assert np.array_equal(dl.cpu().numpy(), l3) and np.array_equal(dm.cpu().numpy(), want[1])
        assert np.array_equal(dk.cpu().numpy().view(np.uint32), want[2])
        eng.lr_check_device(3, dl.data_ptr(), dr.data_ptr(), 0.5, 0.02, False, out_raw_ptr=dl.data_ptr())
        assert np.array_equal(dl.cpu().numpy(), want[0]) and np.array_equal(dr.cpu().numpy(), r3)
        dx = torch.from_numpy(x3).cuda()
        dy = torch.empty_like(dx)
        torch.cuda.synchronize()
        eng.mirror_pair_device(3, dx.data_ptr(), dy.data_ptr())
        assert np.array_equal(dy.cpu().numpy(), lrcheck.mirror_pair(x3))



def _contraction_sensitive_maps(w):
    """One pixel per row whose outcome changes if u - rl*S is evaluated as ONE fused multiply-add: (float)rl * S rounds to the
    integer m while the exact product lies above m by more than an ulp of the small number k.  Rounded separately, xr = u - m = k exactly (t = 0: the partner is R(k)
    alone, which agrees -> kept at tau = 0); fused, xr falls just below k (x0 = k - 1, t ~ 1: the disagreeing neighbour leaks in
    -> inconsistent).  -> (left, right, columns)"""
    s32 = lrcheck.wire_scale()
    cand = np.arange(int(64 / float(s32)), int((w - 80) / float(s32)), dtype=np.int64)
    p32 = cand.astype(np.float32) * s32
    exact = cand.astype(np.float64) * np.float64(s32)                  # 24 x 24 bits: exact in double
    rl = cand[(p32 == np.rint(p32)) & (exact - p32.astype(np.float64) > 8e-6)][:96]      # ulp(k) <= 3.8e-6 for k < 64
    assert len(rl) >= 16
    m = np.rint(rl.astype(np.float32) * s32).astype(np.int64)
    k = 5 + np.arange(len(rl)) % 50
    left = np.zeros((len(rl), w), np.int32)
    right = np.full((len(rl), w), 77, np.int32)
    rows = np.arange(len(rl))
    left[rows, m + k] = rl
    right[rows, k - 1] = rl + 6000
    right[rows, k] = rl
    right[rows, k + 1] = rl + 6000
    fused_xr = ((m + k).astype(np.float64) - rl.astype(np.float64) * np.float64(s32)).astype(np.float32)
    assert np.all(np.floor(fused_xr) == k - 1)                         # what a contracted kernel would compute
    return left, right, m + k


@pytest.mark.gpu
def test_kernel_does_not_contract_the_arithmetic(model_factory):
    """Random maps hardly ever sit on a rounding boundary; these pixels do (see _contraction_sensitive_maps): a kernel whose
    compiler fused a multiply into the following add or subtract rejects them, the contract keeps them."""
    w, h = 1280, 720
    left, right, cols = _contraction_sensitive_maps(w)
    nrow = len(cols)
    L = np.zeros((1, h, w), np.int32)
    R = np.zeros((1, h, w), np.int32)
    L[0, :nrow], R[0, :nrow] = left, right
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)])) as eng:
        for mirrored in (False, True):
            rr = np.ascontiguousarray(R[..., ::-1]) if mirrored else R
            out, mask, kept = eng.lr_check(L, rr, 0.0, 0.0, mirrored)
            w_out, w_mask, w_kept = lrcheck.reference(L, rr, 0.0, 0.0, mirrored, eng.out_scale)
            assert np.all(w_mask[0, np.arange(nrow), cols] == 0) and w_kept.tolist() == [nrow]
            assert np.array_equal(mask, w_mask) and np.array_equal(out, w_out) and np.array_equal(kept, w_kept)


def _pairs(w, h, n, seed=0):
    return np.stack([synth.model_input_i8(w, h, D[(w, h)], seed + k) for k in range(n)])


CASES = [(api.PREC_F16, s) for s in SHAPES] + [(api.PREC_F16X3, s) for s in SHAPES] + [(api.PREC_FP32, SHAPES[0])]


@pytest.mark.gpu
@pytest.mark.parametrize("prec,shape", CASES, ids=[f"{api.PREC_NAMES[p]}-{s[0]}x{s[1]}" for p, s in CASES])
def test_composite_is_the_composition(model_factory, prec, shape):
    w, h = shape
    x = _pairs(w, h, 2)
    with api.StereoNetHIP(model_factory(w, h, D[shape]), max_batch=2, precision=prec) as eng:
        calls0 = eng.refine_stats()["calls"]
        disp, raw, mask, kept, right = eng.infer_lrc(x, 1.0, 0.0, want_right=True)
        assert eng.refine_stats()["calls"] == calls0 + 2     # two forwards
        d_l, r_l = eng.infer(x)
        _, r_m = eng.infer(eng.mirror_pair(x))
        want_disp = d_l.copy()
        want_raw, want_mask, want_kept = eng.lr_check(r_l, r_m, 1.0, 0.0, True, want_disp)
        print(f"{api.PREC_NAMES[prec]} {w}x{h}: kept {kept.tolist()} of {w * h}")
        assert np.array_equal(raw, want_raw) and np.array_equal(mask, want_mask) and np.array_equal(kept, want_kept)
        assert np.array_equal(_bits(disp), _bits(want_disp))
        assert np.array_equal(right, r_m[..., ::-1])
        assert np.all(disp[mask != 0] == 0) and np.all(raw[mask != 0] == 0)
        # a single pair drops the leading dimension and equals the first pair of the batch
        d1, r1, m1, k1 = eng.infer_lrc(x[0], 1.0, 0.0)
        assert np.array_equal(r1, raw[0]) and np.array_equal(m1, mask[0]) and k1.tolist() == kept[:1].tolist()
        assert np.array_equal(_bits(d1), _bits(disp[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1280, 720), (96, 64)])
def test_nv12_input_equals_tensor_input(model_factory, w, h):
    d = D[(w, h)]
    frames = np.stack([synth.sbs_nv12_frame(w, h, d, 20 + k) for k in range(2)])
    with api.StereoNetHIP(model_factory(w, h, d), max_batch=2, precision=api.PREC_F16) as eng:
        tensors = eng.preprocess_sbs_nv12(frames)
        want = eng.infer_lrc(tensors, 1.0, 0.01, want_right=True)
        got = eng.infer_lrc(frames, 1.0, 0.01, want_right=True)
        for g, t in zip(got, want):
            assert np.array_equal(_bits(g) if g.dtype == np.float32 else g, _bits(t) if t.dtype == np.float32 else t)
        one = eng.infer_lrc(frames[0], 1.0, 0.01)             # one flat frame
        assert one[1].shape == (h, w) and np.array_equal(one[1], want[1][0])


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(96, 64), (1280, 720)])
def test_symmetric_input_gives_the_flipped_left_map(model_factory, w, h):
    """A right eye that is the horizontal flip of the left eye makes the mirrored tensor equal the input, so the right eye's
    map must be the flipped, unmasked left map of sn_infer_batch — no oracle involved."""
    x = _pairs(w, h, 1, 30)[0].copy()
    x[3:] = x[:3, :, ::-1]
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), precision=api.PREC_F16) as eng:
        assert np.array_equal(eng.mirror_pair(x), x)
        _, raw_plain = eng.infer(x)
        _, raw, mask, kept, right = eng.infer_lrc(x, 1.0, 0.0, want_right=True)
        assert np.array_equal(right, raw_plain[:, ::-1])
        assert np.array_equal(raw, np.where(mask == 0, raw_plain, 0)) and int(kept[0]) == int((mask == 0).sum())


@pytest.mark.gpu
def test_point_cloud_counts_equal_kept(model_factory):
    w, h = 1280, 720
    x = _pairs(w, h, 2, 40)
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=2, precision=api.PREC_F16) as eng:
        _, raw, mask, kept = eng.infer_lrc(x, 2.0, 0.05)
        _, counts = eng.pointcloud(raw, pointcloud.Camera(), pointcloud.COMPACT)
        assert np.array_equal(counts, kept) and np.array_equal(kept, (raw > 0).reshape(2, -1).sum(1))


@pytest.mark.gpu
def test_device_mode_on_a_caller_stream_equals_host_mode(model_factory):
    import torch
    w, h, n = 1280, 720, 2
    x = _pairs(w, h, n, 50)
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=n, precision=api.PREC_F16) as eng:
        disp, raw, mask, kept, right = eng.infer_lrc(x, 1.0, 0.02, want_right=True)
        dx = torch.from_numpy(x).cuda()
        t_raw = torch.empty((n, h, w), dtype=torch.int32, device="cuda")
        t_right = torch.empty_like(t_raw)
        t_disp = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
        t_mask = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
        t_kept = torch.empty(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s1 = torch.cuda.Stream()
        eng.infer_lrc_device(n, dx.data_ptr(), 1.0, 0.02, t_raw.data_ptr(), t_disp.data_ptr(), t_right.data_ptr(),
                             t_mask.data_ptr(), t_kept.data_ptr(), stream=s1.cuda_stream)
        s1.synchronize()
        assert np.array_equal(t_raw.cpu().numpy(), raw) and np.array_equal(t_right.cpu().numpy(), right)
        assert np.array_equal(_bits(t_disp.cpu().numpy()), _bits(disp)) and np.array_equal(t_mask.cpu().numpy(), mask)
        assert np.array_equal(t_kept.cpu().numpy().view(np.uint32), kept)
        # the float map alone, on the engine's own stream (returns after completion)
        t_disp.fill_(-1.0)
        torch.cuda.synchronize()
        eng.infer_lrc_device(n, dx.data_ptr(), 1.0, 0.02, disp_ptr=t_disp.data_ptr())
        assert np.array_equal(_bits(t_disp.cpu().numpy()), _bits(disp))
        # the two small kernels on the caller's stream
        t_mir = torch.empty_like(dx)
        t_l, t_r = torch.from_numpy(raw).cuda(), torch.from_numpy(right).cuda()
        torch.cuda.synchronize()
        eng.mirror_pair_device(n, dx.data_ptr(), t_mir.data_ptr(), s1.cuda_stream)
        eng.lr_check_device(n, t_l.data_ptr(), t_r.data_ptr(), 0.5, 0.0, False, mask_ptr=t_mask.data_ptr(),
                            kept_ptr=t_kept.data_ptr(), stream=s1.cuda_stream)
        s1.synchronize()
        assert np.array_equal(t_mir.cpu().numpy(), lrcheck.mirror_pair(x))
        _, w_mask, w_kept = lrcheck.reference(raw, right, 0.5, 0.0, False, eng.out_scale)
        assert np.array_equal(t_mask.cpu().numpy(), w_mask) and np.array_equal(t_kept.cpu().numpy().view(np.uint32), w_kept)


@pytest.mark.gpu
def test_argument_errors_leave_the_handle_usable(model_factory):
    w, h = 96, 64
    x = _pairs(w, h, 2, 60)
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=2, precision=api.PREC_F16) as eng:
        before = eng.infer(x)
        lib, hd = eng._lib, eng._h
        l = np.ones((2, h, w), np.int32)
        r = np.ones((2, h, w), np.int32)
        o = np.empty_like(l)
        y = np.empty_like(x)
        dsp = np.empty((2, h, w), np.float32)
        frames = np.zeros(2 * 3 * h * w, np.uint8)
        ok = api.SnLrcParams(1.0, 0.0, 0)
        P = C.byref

        def check(n=1, left=l, right=r, p=ok, out=o, mask=None):
            return lib.sn_lr_check(hd, n, api._np_ptr(left), api._np_ptr(right), P(p) if p is not None else None,
                                   api._np_ptr(out), None, api._np_ptr(mask), None, api.SN_MEM_HOST, None)

        def lrc(n=1, inp=x, kind=0, p=ok, out=o, disp=None, w2=2 * w, hp=h):
            return lib.sn_infer_lrc(hd, n, api._np_ptr(inp), kind, w2, hp, P(p) if p is not None else None, api._np_ptr(out),
                                    api._np_ptr(disp), None, None, None, api.SN_MEM_HOST, None)

        def mirror(n=1, inp=x, out=y):
            return lib.sn_mirror_pair_i8(hd, n, api._np_ptr(inp), api._np_ptr(out), api.SN_MEM_HOST, None)

        assert check() == 0 and lrc() == 0 and lrc(out=None, disp=dsp) == 0 and mirror() == 0 and lrc(inp=frames, kind=1) == 0
        bad_p = [None, api.SnLrcParams(-1.0, 0.0, 0), api.SnLrcParams(0.0, -0.5, 0), api.SnLrcParams(float("nan"), 0.0, 0),
                 api.SnLrcParams(1.0, float("nan"), 0), api.SnLrcParams(float("inf"), 0.0, 0)]
        for p in bad_p:
            assert check(p=p) == -1 and lrc(p=p) == -1
        for n in (0, -1, 3):
            assert check(n=n) == -1 and lrc(n=n) == -1 and mirror(n=n) == -1
        assert check(left=None) == -1 and check(right=None) == -1 and check(out=None, mask=None) == -1
        assert lrc(inp=None) == -1 and lrc(out=None, disp=None) == -1
        assert lrc(kind=2) == -1 and lrc(kind=-1) == -1
        assert lrc(inp=frames, kind=1, w2=w) == -1 and lrc(inp=frames, kind=1, hp=h + 2) == -1
        assert mirror(inp=None) == -1 and mirror(out=None) == -1 and mirror(out=x) == -1        # in == out overlaps
        assert "sn_mirror_pair_i8" in lib.sn_last_error(hd).decode()
        with pytest.raises(api.StereoNetError):
            eng.lr_check(l[:, :-1], r[:, :-1])
        with pytest.raises(api.StereoNetError):
            eng.infer_lrc(np.zeros(7, np.uint8))
        after = eng.infer(x)
        assert np.array_equal(after[1], before[1]) and np.array_equal(_bits(after[0]), _bits(before[0]))


@pytest.mark.gpu
def test_filelist_lrc(model_factory, tmp_path, capsys):
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
    assert filelist.main(base + ["--out", str(tmp_path / "lrc"), "--gt", str(tmp_path / "gt.list"), "--lrc", "1"]) == 0
    lrc_summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    with pytest.raises(SystemExit):
        filelist.main(base + ["--lrc", "1,-2"])
    capsys.readouterr()
    assert plain_summary == {"frames": 2}                                      # without the flag: the summary of before
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(f"{i}.{e}" for i in (0, 1) for e in ("raw.bin", "disp.pfm", "depth.ppm"))
    assert sorted(os.listdir(tmp_path / "lrc")) == sorted(f"{i}.{e}" for i in (0, 1)
                                                          for e in ("raw.bin", "disp.pfm", "depth.ppm", "mask.pgm"))
    densities = []
    with api.StereoNetHIP(model, precision=api.PREC_F16) as eng:
        for i in range(2):
            eyes = [images.bgr_to_nv12(images.imread_bgr(names[s][i])) for s in ("l", "r")]
            sbs = images.sbs_from_eyes(eyes[0], eyes[1], w, h)
            # without the flag every file is what the unchanged code path writes from infer_sbs_nv12
            disp, raw = eng.infer_sbs_nv12(sbs)
            images.write_pfm(str(tmp_path / "want.pfm"), disp)
            _, depth = render.disparity_and_depth(raw.view(np.uint32))
            images.write_ppm(str(tmp_path / "want.ppm"), render.colorize_depth(depth)[..., ::-1])
            rd = lambda p: open(p, "rb").read()      # noqa: E731
            assert rd(tmp_path / "plain" / f"{i}.raw.bin") == raw.tobytes()
            assert rd(tmp_path / "plain" / f"{i}.disp.pfm") == rd(tmp_path / "want.pfm")
            assert rd(tmp_path / "plain" / f"{i}.depth.ppm") == rd(tmp_path / "want.ppm")
            # with it: the masked map of infer_lrc, the mask beside it
            mdisp, mraw, mask, kept = eng.infer_lrc(sbs, 1.0, 0.0)
            assert rd(tmp_path / "lrc" / f"{i}.raw.bin") == mraw.tobytes()
            assert np.array_equal(images.read_pnm(str(tmp_path / "lrc" / f"{i}.mask.pgm")), mask)
            assert np.array_equal(_bits(images.read_pfm(str(tmp_path / "lrc" / f"{i}.disp.pfm"))), _bits(mdisp))
            assert np.array_equal(mraw, np.where(mask == 0, raw, 0))
            densities.append(float(kept[0]) / (w * h))
        recs = filelist.run_imglist(eng, str(tmp_path / "l.list"), str(tmp_path / "r.list"), gt_list=str(tmp_path / "gt.list"),
                                    lrc=(1.0, 0.0))
        gt = synth.disparity_field(w, h, d)
        for rec in recs:
            assert rec["metrics"]["valid_px"] == int(((rec["mask"] == 0) & (gt < d)).sum())      # kept and valid ground truth
    assert lrc_summary["frames"] == 2 and lrc_summary["density"] == pytest.approx(np.mean(densities), abs=1e-12)
    assert set(lrc_summary) == {"frames", "epe", "bad1", "bad3", "d1", "density"}
