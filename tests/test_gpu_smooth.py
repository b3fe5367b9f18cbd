"""sn_smooth_raw on the MI355X: the kernel equals the numpy twin (hobot_stereonet_amd/smooth.py) bit for bit — out, mask, counts
and the float map's bits — on maps built to reach every class of pixel, for both guide forms, in every buffer mode, batched
and in place; argument errors, determinism, the composition with sn_infer_lrc / sn_filter_raw / depth / point cloud, and the
file-list harness's --smooth.  Every input is run once; the twin's answers are computed once per (shape, setting) and shared.

Two conditions keep the comparison from passing vacuously.  The scene's mask must hold every value the setting can produce:
0, 1, 128 and 129 when min_valid > 0; without filling (min_valid == 0) 129 cannot occur and {0, 1, 128} is the whole set.  The
spike map must hold an invalid pixel with >= min_valid measured neighbours that stays 0 because every weight is 0; that needs
sigma_luma > 0 (at sigma_luma == 0 every weight is 1) and min_valid > 0."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from hobot_stereonet_amd import api, dispfilter, pointcloud, smooth, synth

D = {(96, 64): 48, (1242, 375): 256}
IMAX, IMIN = 2 ** 31 - 1, -2 ** 31
SETTINGS = [(1, 0, 0), (2, 0, 5), (2, 12, 5), (1, 1, 1)]          # (radius, sigma_luma, min_valid)
CASES = [(96, 64, s) for s in SETTINGS + [(3, 4, 25)]] + [(1242, 375, s) for s in SETTINGS]
NAMES = ("scene", "constant", "checkerboard", "all-invalid", "corner values", "spikes")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _maps(w, h):
    """-> (maps int32 (6,h,w), luma uint8 (6,h,w)) in the order of NAMES"""
    rng = np.random.default_rng(w * 7 + h)
    y, x = np.mgrid[0:h, 0:w]
    scene, scene_luma, _ = smooth.noisy_scene(w, h, w + h)
    texture = rng.integers(0, 256, (h, w)).astype(np.uint8)
    constant = np.full((h, w), 63000, np.int32)
    checker = np.where((x + y) % 2 == 0, 30000 + 7 * x + 3 * y, 0).astype(np.int32)
    vals = np.array([IMIN, -7, -1, 0, 0, 1, 1, 2, IMAX, IMAX - 1, 1000, 1000, 1001], np.int64)
    corners = vals[rng.integers(0, len(vals), (h, w))].astype(np.int32)
    corners[0, :6] = [IMAX, 1, IMAX, IMIN, 1, 2]
    corners[-1, -4:] = [1, IMAX, 0, IMAX]
    coarse = ((x // 5 + y // 3) % 4 * 60).astype(np.uint8)            # flat luma cells: many equal weights, many ties
    spikes = (20000 + rng.integers(0, 400, (h, w))).astype(np.int32)
    hole = (x % 5 == 2) & (y % 5 == 2)
    spikes[hole] = np.where(rng.random(int(hole.sum())) < 0.3, -9, 0)
    spike_luma = np.zeros((h, w), np.uint8)
    spike_luma[hole & ((x // 5 + y // 5) % 2 == 0)] = 255             # half the holes: no neighbour has a weight > 0
    spike_luma[(x % 11 == 0) & (y % 7 == 0)] = 255                    # and some measured pixels: their own only participant
    maps = np.stack([scene, constant, checker, np.zeros((h, w), np.int32), corners, spikes])
    luma = np.stack([scene_luma, texture, texture[::-1].copy(), texture, coarse, spike_luma])
    maps.setflags(write=False)
    luma.setflags(write=False)
    return maps, luma


@functools.lru_cache(maxsize=None)
def _want(w, h, setting):
    maps, luma = _maps(w, h)
    out, mask, counts = smooth.reference(maps, luma, *setting)
    for a in (out, mask, counts):
        a.setflags(write=False)
    return out, mask, counts


def _tensor(luma):
    """int8 model inputs (n,6,h,w) whose channel 0 carries `luma`; the other channels are noise"""
    rng = np.random.default_rng(int(luma[0, 0, 0]) + luma.shape[-1])
    t = rng.integers(-128, 128, (luma.shape[0], 6) + luma.shape[1:]).astype(np.int8)
    t[:, 0] = (luma ^ np.uint8(0x80)).view(np.int8)
    return t


def _nv12(luma, pitch):
    """NV12 frames of `pitch` (noise in the chroma rows and beside the left eye) whose luma rows carry `luma`"""
    n, h, w = luma.shape
    rng = np.random.default_rng(pitch + n)
    frames = rng.integers(0, 256, (n, h + (h + 1) // 2, pitch)).astype(np.uint8)
    frames[:, :h, :w] = luma
    return frames.reshape(-1)


def _check(tag, got, want, disp, disp0, sel=slice(None)):
    out, mask, counts = got
    w_out, w_mask, w_counts = (a[sel] for a in want)
    print(f"{tag}: counts {counts.tolist()}, differing pixels (out, mask) = {int((out != w_out).sum())}, {int((mask != w_mask).sum())}")
    assert np.array_equal(mask, w_mask), tag
    assert np.array_equal(out, w_out), tag
    assert np.array_equal(counts, w_counts), tag
    if disp is not None:                                             # untouched words keep their random bit pattern
        assert np.array_equal(_bits(disp), _bits(smooth.expected_disp(disp0, w_out, w_mask))), tag


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,setting", CASES, ids=[f"{w}x{h}-r{s[0]}-s{s[1]}-m{s[2]}" for w, h, s in CASES])
def test_smooth_kernel_equals_twin_bit_for_bit(model_factory, w, h, setting):
    radius, sigma, min_valid = setting
    maps, luma = _maps(w, h)
    want = _want(w, h, setting)
    scene_mask, spike_mask = want[1][0], want[1][5]
    share = float((scene_mask & 128 != 0).mean())
    print(f"{w}x{h} {setting}: scene mask {dict(zip(*[a.tolist() for a in np.unique(scene_mask, return_counts=True)]))}, "
          f"changed share {share:.2f}")
    assert set(np.unique(scene_mask).tolist()) == ({0, 1, 128, 129} if min_valid else {0, 1, 128})
    if sigma and min_valid:
        pad = np.pad(maps[5] > 0, radius)
        measured = sum(pad[dy:dy + h, dx:dx + w].astype(np.int32) for dy in range(2 * radius + 1) for dx in range(2 * radius + 1))
        starved = (spike_mask == 1) & (measured >= min_valid)
        print(f"  spikes: {int(starved.sum())} invalid pixels with >= {min_valid} measured neighbours stay 0")
        assert starved.any() and (spike_mask == 129).any()
    rng = np.random.default_rng(w + h + radius)
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=3) as eng:
        for sel, kind in ((slice(0, 3), api.SN_GUIDE_NV12), (slice(3, 6), api.SN_GUIDE_TENSOR)):
            disp0 = rng.integers(0, 2 ** 32, (3, h, w), dtype=np.uint32).view(np.float32)
            disp = disp0.copy()
            guide = _nv12(luma[sel], w) if kind == api.SN_GUIDE_NV12 else _tensor(luma[sel])
            got = eng.smooth_raw(maps[sel], guide, kind, 0, radius, sigma, min_valid, disp=disp)
            _check(f"{w}x{h} {setting} {NAMES[sel]}", got, want, disp, disp0, sel)
        assert want[2][1].tolist() == [w * h, 0, 0] and want[2][3].tolist() == [0, 0, 0]      # constant: a fixed point; all-invalid


@pytest.mark.gpu
def test_smooth_guide_forms_give_the_same_bytes(model_factory):
    w, h, setting = 96, 64, (2, 12, 5)
    maps, luma = _maps(w, h)
    sel = slice(4, 6)
    want = _want(w, h, setting)
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=2) as eng:
        results = []
        for kind, guide, pitch in ((api.SN_GUIDE_TENSOR, _tensor(luma[sel]), 0), (api.SN_GUIDE_NV12, _nv12(luma[sel], w), w),
                                   (api.SN_GUIDE_NV12, _nv12(luma[sel], 2 * w), 2 * w)):
            got = eng.smooth_raw(maps[sel], guide, kind, pitch, *setting)
            _check(f"guide kind {kind} pitch {pitch}", got, want, None, None, sel)
            results.append(b"".join(a.tobytes() for a in got))
        assert results[0] == results[1] == results[2]
        # one map: the luma rows alone, without chroma rows behind them, are a whole guide
        got = eng.smooth_raw(maps[5], np.ascontiguousarray(luma[5]), api.SN_GUIDE_NV12, w, *setting)
        _check("luma rows only", (got[0][None], got[1][None], got[2]), want, None, None, slice(5, 6))
        # sigma_luma == 0 reads no guide: none at all, or one of any content
        plain = eng.smooth_raw(maps[sel], None, api.SN_GUIDE_NV12, 0, 2, 0, 5)
        _check("no guide", plain, _want(w, h, (2, 0, 5)), None, None, sel)


@pytest.mark.gpu
def test_smooth_device_mode_in_place_partial_outputs_and_slices(model_factory):
    import torch
    w, h, n, setting = 96, 64, 9, (2, 12, 5)                        # 9 maps: past the scratch's slice of 8
    maps6, luma6 = _maps(w, h)
    order = [0, 4, 5, 2, 1, 3, 5, 0, 4]
    maps, luma = np.ascontiguousarray(maps6[order]), np.ascontiguousarray(luma6[order])
    want = tuple(a[order] for a in _want(w, h, setting))
    rng = np.random.default_rng(11)
    disp0 = rng.integers(0, 2 ** 32, maps.shape, dtype=np.uint32).view(np.float32)
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=n) as eng:
        hdisp = disp0.copy()
        host = eng.smooth_raw(maps, _nv12(luma, 2 * w), api.SN_GUIDE_NV12, 2 * w, *setting, disp=hdisp)
        _check("host mode n=9", host, want, hdisp, disp0)
        hw = h * w
        pad = torch.full((n * hw + 8,), -3, dtype=torch.int32, device="cuda")       # raw at an offset of 4 words, guarded
        d_raw = pad[4:4 + n * hw]
        d_raw.copy_(torch.from_numpy(maps).reshape(-1))
        d_guide = torch.from_numpy(_tensor(luma)).cuda()
        d_out = torch.full((n * hw + 2,), -3, dtype=torch.int32, device="cuda")
        d_mask = torch.full((n * hw + 2,), 77, dtype=torch.uint8, device="cuda")
        d_disp = torch.from_numpy(disp0.copy()).cuda()
        d_cnt = torch.full((n, 3), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s1 = torch.cuda.Stream()
        args = (n, d_raw.data_ptr(), d_guide.data_ptr(), api.SN_GUIDE_TENSOR, 0) + setting

        def fetched(t, count, dtype):
            a = t.cpu().numpy()
            assert np.all(a[:1] == a[-1:]) and a[0] in (-3, 77)      # the guard words around the output
            return a[1:1 + count].reshape(n, h, w).astype(dtype, copy=False)

        eng.smooth_raw_device(*args, out_raw_ptr=d_out.data_ptr() + 4, mask_ptr=d_mask.data_ptr() + 1, disp_ptr=d_disp.data_ptr(),
                              counts_ptr=d_cnt.data_ptr(), stream=s1.cuda_stream)
        s1.synchronize()
        assert np.array_equal(d_raw.cpu().numpy().reshape(maps.shape), maps)      # the input is only read
        dev = (fetched(d_out, n * hw, np.int32), fetched(d_mask, n * hw, np.uint8), d_cnt.cpu().numpy().view(np.uint32))
        _check("device mode, caller stream", dev, want, d_disp.cpu().numpy(), disp0)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(dev, host))
        # mask and counts only, on the smoother's own stream (returns after completion); then out_raw only
        d_mask.fill_(77), d_cnt.fill_(-1), d_out.fill_(-3)
        torch.cuda.synchronize()
        eng.smooth_raw_device(*args, mask_ptr=d_mask.data_ptr() + 1, counts_ptr=d_cnt.data_ptr())
        assert np.array_equal(fetched(d_mask, n * hw, np.uint8), want[1])
        assert np.array_equal(d_cnt.cpu().numpy().view(np.uint32), want[2]) and np.all(d_out.cpu().numpy() == -3)
        eng.smooth_raw_device(*args, out_raw_ptr=d_out.data_ptr() + 4, stream=s1.cuda_stream)
        s1.synchronize()
        assert np.array_equal(fetched(d_out, n * hw, np.int32), want[0])
        # in place: out_raw == raw, all nine maps, on the caller's stream
        d_mask.fill_(77)
        torch.cuda.synchronize()
        eng.smooth_raw_device(*args, out_raw_ptr=d_raw.data_ptr(), mask_ptr=d_mask.data_ptr() + 1, stream=s1.cuda_stream)
        s1.synchronize()
        assert np.array_equal(d_raw.cpu().numpy().reshape(maps.shape), want[0])
        assert np.array_equal(fetched(d_mask, n * hw, np.uint8), want[1])
        assert np.all(pad[:4].cpu().numpy() == -3) and np.all(pad[4 + n * hw:].cpu().numpy() == -3)
        # host mode with out == raw is the same call through the staging
        lib, inplace = eng._lib, maps.copy()
        p = api.SnSmoothParams(*setting)
        g = _tensor(luma)
        assert lib.sn_smooth_raw(eng._h, n, inplace.ctypes.data, g.ctypes.data, api.SN_GUIDE_TENSOR, 0, C.byref(p),
                                 inplace.ctypes.data, None, None, None, api.SN_MEM_HOST, None) == 0
        assert np.array_equal(inplace, want[0])


@pytest.mark.gpu
def test_smooth_batch_equals_single_calls_and_is_deterministic(model_factory):
    w, h, setting = 96, 64, (3, 4, 25)
    maps6, luma6 = _maps(w, h)
    sel = [0, 4, 5]
    maps, luma = np.ascontiguousarray(maps6[sel]), np.ascontiguousarray(luma6[sel])
    guide = _tensor(luma)
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=3) as eng:
        batch = eng.smooth_raw(maps, guide, api.SN_GUIDE_TENSOR, 0, *setting)
        _check("n=3", batch, tuple(a[sel] for a in _want(w, h, setting)), None, None)
        for k in range(3):
            one = eng.smooth_raw(maps[k], guide[k], api.SN_GUIDE_TENSOR, 0, *setting)
            assert one[0].shape == (h, w) and one[2].shape == (1, 3)
            assert np.array_equal(one[0], batch[0][k]) and np.array_equal(one[1], batch[1][k]) and np.array_equal(one[2][0], batch[2][k])
        again = eng.smooth_raw(maps, guide, api.SN_GUIDE_TENSOR, 0, *setting)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(batch, again))


@pytest.mark.gpu
def test_smooth_argument_errors_leave_the_outputs_and_the_handle_untouched(model_factory):
    w, h = 96, 64
    x = np.stack([synth.model_input_i8(w, h, D[(w, h)], 60 + k) for k in range(2)])
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=2, precision=api.PREC_F16) as eng:
        before = eng.infer(x)
        lib, hd = eng._lib, eng._h
        buf = np.ones((4, h, w), np.int32)                    # raw = buf[:2], out = buf[2:]: one allocation, to build overlaps
        raw, out = buf[:2], buf[2:]
        out[:] = -5
        mask = np.full((2, h, w), 99, np.uint8)
        dsp = np.full((2, h, w), 7.0, np.float32)
        cnt = np.full((2, 3), 12345, np.uint32)
        nv = np.zeros(2 * (h + h // 2) * 2 * w + 2 * h * w * 4, np.uint8)      # two frames of any pitch up to 2w, and room to alias
        ten = np.zeros((2, 6, h, w), np.int8)
        ok = api.SnSmoothParams(2, 12, 5)

        def call(n=1, r=raw, g=nv, kind=api.SN_GUIDE_NV12, pitch=w, p=ok, o=out, m=None, d=None, c=None, mem=api.SN_MEM_HOST):
            ptr = lambda a: a if isinstance(a, int) or a is None else a.ctypes.data      # noqa: E731
            return lib.sn_smooth_raw(hd, n, ptr(r), ptr(g), kind, pitch, C.byref(p) if p is not None else None, ptr(o), ptr(d),
                                     ptr(m), ptr(c), mem, None)

        def failed(rc):
            return rc == -1 and "sn_smooth_raw" in lib.sn_last_error(hd).decode()

        bad = []
        for n in (0, -1, 3):
            bad.append(call(n=n, m=mask, d=dsp, c=cnt))
        bad += [call(p=None), call(r=None), call(o=None, m=None), call(mem=2)]
        for prm in ((0, 12, 0), (4, 12, 0), (-1, 0, 0), (2, -1, 0), (2, 256, 0), (2, 12, -1), (2, 12, 26), (1, 0, 10), (3, 0, 50)):
            bad.append(call(p=api.SnSmoothParams(*prm), m=mask, d=dsp, c=cnt))
        bad += [call(g=None), call(g=None, kind=api.SN_GUIDE_TENSOR)]                       # sigma_luma > 0 without a guide
        bad += [call(kind=2), call(kind=-1), call(kind=2, g=None, p=api.SnSmoothParams(2, 0, 0))]
        bad += [call(pitch=w - 2), call(pitch=w + 1), call(pitch=0), call(pitch=-w)]
        assert all(failed(rc) for rc in bad), bad
        # any overlap but out_raw == raw; the guide must not overlap an output
        over = [call(n=2, o=raw.ctypes.data + 4 * h * w), call(n=1, o=None, m=raw.view(np.uint8)), call(n=1, d=raw.view(np.float32)),
                call(n=1, d=out.view(np.float32)), call(n=1, c=out.view(np.uint32)), call(n=1, m=mask, c=mask.view(np.uint32)),
                call(n=1, m=mask, d=dsp, c=dsp.view(np.uint32)), call(n=1, g=out.view(np.uint8)), call(n=1, o=None, m=nv),
                call(n=2, g=ten, kind=api.SN_GUIDE_TENSOR, o=None, m=ten.view(np.uint8).reshape(-1)[6 * h * w:]),
                call(n=1, g=raw.view(np.uint8), o=raw)]
        assert all(failed(rc) for rc in over), over
        assert "overlap" in lib.sn_last_error(hd).decode()
        # nothing was written by any failed call
        assert np.all(out == -5) and np.all(raw == 1) and np.all(mask == 99) and np.all(dsp == 7.0) and np.all(cnt == 12345)
        # the bounds themselves are allowed, as are in place, a guide beside (not in) the outputs, and no guide at sigma_luma 0
        assert call() == 0 and call(n=2, o=None, m=mask, c=cnt) == 0 and call(n=2, m=mask, d=dsp, c=cnt) == 0
        assert call(n=2, o=raw) == 0 and call(n=2, g=raw.view(np.uint8), o=out) == 0
        for prm in ((1, 0, 9), (3, 255, 49), (1, 1, 0)):
            assert call(p=api.SnSmoothParams(*prm)) == 0, prm
        assert call(g=None, p=api.SnSmoothParams(2, 0, 0)) == 0 and call(g=None, pitch=0, p=api.SnSmoothParams(2, 0, 0)) == 0
        assert call(n=2, g=ten, kind=api.SN_GUIDE_TENSOR, pitch=-1) == 0                     # guide_pitch is ignored for the tensor
        assert call(pitch=2 * w) == 0
        with pytest.raises(api.StereoNetError):
            eng.smooth_raw(raw[:, :-1], None, sigma_luma=0)
        with pytest.raises(api.StereoNetError):
            eng.smooth_raw(raw, None, sigma_luma=0, disp=np.zeros((2, h, w), np.float64))
        with pytest.raises(api.StereoNetError):
            eng.smooth_raw(np.ones((3, h, w), np.int32), None, sigma_luma=0)
        with pytest.raises(api.StereoNetError):
            eng.smooth_raw(raw, np.zeros(h * w, np.uint8))                                   # two maps, one frame of luma
        with pytest.raises(api.StereoNetError):
            eng.smooth_raw(raw, ten[0], api.SN_GUIDE_TENSOR)
        after = eng.infer(x)                                                 # existing calls are unchanged by all of this
        assert np.array_equal(after[1], before[1]) and np.array_equal(_bits(after[0]), _bits(before[0]))


@pytest.mark.gpu
def test_smooth_composes_with_lrc_filter_depth_and_point_cloud(model_factory):
    w, h, n = 96, 64, 2
    x = np.stack([synth.model_input_i8(w, h, D[(w, h)], 80 + k) for k in range(n)])
    setting = (2, 12, 5)
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=n, precision=api.PREC_F16) as eng:
        plain_before = eng.infer(x)
        disp, raw, lmask, kept = eng.infer_lrc(x, 1.0, 0.0)
        fout, fmask, fcounts = eng.filter_raw(raw, 200, 1.0, 16, disp=disp)
        sdisp = disp.copy()
        out, smask, counts = eng.smooth_raw(fout, x, api.SN_GUIDE_TENSOR, 0, *setting, disp=sdisp)
        want = smooth.reference(fout, smooth.luma_from_tensor(x), *setting, out_scale=eng.out_scale)
        print(f"kept {kept.tolist()}, after the filter {fcounts.tolist()}, after the smoother {counts.tolist()}")
        _check("after lrc and filter", (out, smask, counts), want, sdisp, disp)
        assert (smask & 128).any()
        depth = eng.depth_from_raw(out)
        assert np.array_equal(np.isfinite(depth), out > 0)
        _, pc_counts = eng.pointcloud(out, pointcloud.Camera(), pointcloud.COMPACT)
        assert np.array_equal(pc_counts, counts[:, 0])
        # the three masks share INVALID_IN (1) and nothing else: their OR can be taken apart again
        both = lmask | fmask | smask
        assert np.array_equal(both & 0x0e, lmask & 0x0e) and np.array_equal(both & 0x30, fmask & 0x30)
        assert np.array_equal(both & 0x80, smask & 0x80) and not (both & 0x40).any()
        assert not ((lmask | fmask) & 0x80).any() and not ((lmask | smask) & 0x30).any() and not ((fmask | smask) & 0x0e).any()
        assert np.array_equal(smask & 1 != 0, fout <= 0)
        plain_after = eng.infer(x)
        for a, b in zip(plain_before, plain_after):                          # existing calls: identical bytes around the call
            assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_filelist_smooth(model_factory, tmp_path, capsys):
    from hobot_stereonet_amd import filelist, images
    w, h, d = 96, 64, 48
    model = model_factory(w, h, d)
    names = {"l": [], "r": []}
    for k in range(2):
        lt, rt = synth.stereo_pair_u8(w, h, d, 70 + k)
        for side, eye in (("l", lt), ("r", rt)):
            p = str(tmp_path / f"{side}{k}.png")
            images.write_png(p, np.ascontiguousarray(eye.transpose(1, 2, 0)))
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
    assert filelist.main(base + ["--out", str(tmp_path / "o"), "--gt", str(tmp_path / "gt.list"), "--lrc", "1", "--fill", "16",
                                 "--smooth", "2,12,5"]) == 0
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert sorted(os.listdir(tmp_path / "o")) == sorted(
        f"{i}.{e}" for i in (0, 1) for e in ("raw.bin", "disp.pfm", "depth.ppm", "mask.pgm", "filter.pgm", "smooth.pgm"))
    smoothed, densities = 0, []
    with api.StereoNetHIP(model, precision=api.PREC_F16) as eng:
        recs = filelist.run_imglist(eng, str(tmp_path / "l.list"), str(tmp_path / "r.list"), gt_list=str(tmp_path / "gt.list"),
                                    lrc=(1.0, 0.0), flt=(0, 1.0, 16), smooth=(2, 12, 5))
        for i in range(2):
            eyes = [images.bgr_to_nv12(images.imread_bgr(names[s][i])) for s in ("l", "r")]
            sbs = images.sbs_from_eyes(eyes[0], eyes[1], w, h)
            mdisp, mraw, lmask, kept = eng.infer_lrc(sbs, 1.0, 0.0)
            f_out, f_mask, _ = dispfilter.reference(mraw, 0, 1.0, 16, out_scale=eng.out_scale)      # the map before the step
            f_disp = _bits(np.where(f_mask != 0, np.where(f_out > 0, f_out.astype(np.float32) * dispfilter.wire_scale(eng.out_scale),
                                                          np.float32(0)), mdisp)).view(np.float32)
            luma = smooth.luma_from_nv12(sbs, w, h, 2 * w)[0]
            w_out, w_mask, w_counts = smooth.reference(f_out, luma, 2, 12, 5, out_scale=eng.out_scale)
            assert open(tmp_path / "o" / f"{i}.raw.bin", "rb").read() == w_out.tobytes()
            assert np.array_equal(images.read_pnm(str(tmp_path / "o" / f"{i}.smooth.pgm")), w_mask)
            assert np.array_equal(images.read_pnm(str(tmp_path / "o" / f"{i}.filter.pgm")), f_mask)
            assert np.array_equal(_bits(images.read_pfm(str(tmp_path / "o" / f"{i}.disp.pfm"))),
                                  _bits(smooth.expected_disp(f_disp, w_out, w_mask, eng.out_scale)))
            rec = recs[i]
            assert np.array_equal(rec["raw"], w_out) and np.array_equal(rec["smooth_mask"], w_mask)
            assert rec["smoothed"] == int(w_counts[0, 1]) + int(w_counts[0, 2]) == int((w_mask & 128 != 0).sum()) > 0
            assert rec["density"] == float(w_counts[0, 0]) / (w * h) == float((w_out > 0).sum()) / (w * h)
            assert rec["smooth_epe"]["valid_px"] == int(((f_out > 0) & (synth.disparity_field(w, h, d) < d)).sum())
            assert np.isfinite(rec["smooth_epe"]["before"]) and np.isfinite(rec["smooth_epe"]["after"])
            smoothed += rec["smoothed"]
            densities.append(rec["density"])
    assert {"smoothed", "density", "smooth_epe_before", "smooth_epe_after", "filled"} <= set(summary)
    assert summary["frames"] == 2 and summary["smoothed"] == smoothed
    assert summary["density"] == pytest.approx(np.mean(densities), abs=1e-12)
