"""sn_filter_raw on the MI355X: the kernels equal the numpy twin (hobot_stereonet_amd/dispfilter.py) bit for bit on maps built to
reach every class and every path of the labelling (components across every tile border, one component of H*W pixels, a
serpentine, one component per pixel), device mode on a caller stream and in place, argument errors, determinism, the
composition with sn_infer_lrc / the point cloud / the depth, and the file-list harness's --speckle / --fill.  Every input is
run once."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from hobot_stereonet_amd import api, dispfilter, pointcloud, synth

SHAPES = [(96, 64), (1242, 375), (1280, 720)]
D = {(96, 64): 48, (1242, 375): 256, (1280, 720): 192}
S32 = dispfilter.wire_scale()
S = float(S32)
IMAX = 2 ** 31 - 1
TILE_W, TILE_H = 64, 16              # the labelling kernel's tile: speckles are placed on its corners and borders
# (speckle_max_px, speckle_diff_px, fill_max_px): speckle only, fill only, both
PARAMS = [(6, 1.0, 0), (0, 1.0, 16), (40, 0.5, 16)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _scene(w, h, mx, seed):
    """A piecewise-smooth scene (a slanted background and two foreground slabs: components that span every tile), about 30 %
    rejected in strips and blobs, and isolated speckles of 1 .. mx + 1 pixels on tile corners and borders.
    -> (map, [(size, y, x) of every speckle])"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    d = 12.0 + 0.02 * x + 0.01 * y
    d[(x > 0.25 * w) & (x < 0.5 * w) & (y > 0.2 * h)] += 30.0
    d[(x > 0.7 * w) & (y < 0.6 * h)] += 14.0 + 0.03 * y[(x > 0.7 * w) & (y < 0.6 * h)]
    m = np.rint(d / S).astype(np.int32)
    strips = ((0.25 * w - 12, 12), (0.7 * w - 25, 25), (0.55 * w, 5), (0.1 * w, 17), (w - 9, 9), (0, 7)) if w >= 400 else \
             ((0.25 * w - 5, 5), (0.7 * w - 9, 9), (w - 3, 3), (0, 2))
    for x0, width in strips:                                             # fillable and not, at both image borders
        m[:, int(x0):int(x0) + width] = 0
    rmax = max(4, min(w, h) // 10)
    for _ in range(int(0.22 * w * h * 3 / (np.pi * rmax * rmax))):       # blobs: about a fifth of the image
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(2, rmax)
        m[(y - cy) ** 2 + (x - cx) ** 2 <= r * r] = 0
    m[rng.random((h, w)) < 0.03] = 0                                     # single rejected pixels
    m[rng.random((h, w)) < 0.002] = -5
    sizes = [mx, mx + 1, 1] + (list(range(2, mx)) if mx <= 8 else [2, 7, mx - 1])
    placed = []
    rw = 9                                                               # a speckle is rows of 9 pixels and a remainder
    anchors = [(ty * TILE_H, tx * TILE_W) for ty in range(1, -(-h // TILE_H)) for tx in range(1, -(-w // TILE_W))]
    rng.shuffle(anchors)
    for i, (ay, ax) in enumerate(anchors[:3 * len(sizes)]):
        size = sizes[i % len(sizes)]
        rows = -(-size // rw)
        y0, x0 = ay - min(rows // 2, 1) - (i % 2), ax - 4 + (i % 3 == 0) * 4      # across the corner, or along a border
        if y0 < 2 or x0 < 2 or y0 + rows + 2 > h or x0 + rw + 2 > w:
            continue
        m[y0 - 1:y0 + rows + 1, x0 - 1:x0 + rw + 1] = 0
        val = int(round((70.0 + i) / S))
        for k in range(size):
            m[y0 + k // rw, x0 + k % rw] = val + 10 * k
        placed.append((size, y0, x0))
    return m, placed


def _constant(w, h):
    return np.full((h, w), int(round(33.0 / S)), np.int32)


def _serpentine(w, h):
    """A one-pixel path through the whole image: every second row, joined at alternating ends."""
    m = np.zeros((h, w), np.int32)
    m[::2] = 40000 + 3 * np.arange(w, dtype=np.int32)[None, :]
    m[1::4, -1] = 40000 + 3 * (w - 1)
    m[3::4, 0] = 40000
    return m


def _checkerboard(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return np.where((x + y) % 2 == 0, 30000 + x + y, 0).astype(np.int32)


def _corners(w, h, seed):
    """int32 corner values side by side: differences that only fit 64 bits, and pairs exactly at and beyond the threshold"""
    rng = np.random.default_rng(seed)
    vals = np.array([-2 ** 31, -7, 0, 1, 2, IMAX, IMAX - 1, 1999, 2000, 2001, 4000, 999, 1000], np.int64)
    m = vals[rng.integers(0, len(vals), (h, w))].astype(np.int32)
    m[0, :6] = [IMAX, 1, IMAX, -2 ** 31, 1, 2]
    m[-1, -4:] = [1, IMAX, 0, IMAX]
    return m


def _maps(w, h, mx, seed):
    scene, placed = _scene(w, h, mx, seed)
    return np.stack([scene, _constant(w, h), _serpentine(w, h), _checkerboard(w, h), np.zeros((h, w), np.int32),
                     _corners(w, h, seed + 1)]), placed


def _expected_disp(disp0, out, mask):
    val = np.where(out > 0, out.astype(np.float32) * S32, np.float32(0))
    return np.where(mask != 0, _bits(val), _bits(disp0))


def _run_and_compare(eng, maps, params, rng, tag):
    disp0 = rng.integers(0, 2 ** 32, maps.shape, dtype=np.uint32).view(np.float32)
    disp = disp0.copy()
    out, mask, counts = eng.filter_raw(maps, *params, disp=disp)
    w_out, w_mask, w_counts = dispfilter.reference(maps, *params, out_scale=eng.out_scale)
    nbad = int((out != w_out).sum()), int((mask != w_mask).sum())
    print(f"{tag}: counts {counts.tolist()}, differing pixels (out, mask) = {nbad}")
    assert np.array_equal(mask, w_mask), tag
    assert np.array_equal(out, w_out), tag
    assert np.array_equal(counts, w_counts), tag
    assert np.array_equal(_bits(disp), _expected_disp(disp0, w_out, w_mask)), tag
    return w_out, w_mask, w_counts


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SHAPES)
def test_filter_kernels_equal_twin_bit_for_bit(model_factory, w, h):
    rng = np.random.default_rng(w * 3 + h)
    seen = set()
    small = (w, h) == SHAPES[0]
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=9 if small else 3) as eng:
        for params in PARAMS:
            mx = params[0]
            maps, placed = _maps(w, h, mx or 6, w + h + mx)
            frac = float((maps[0] <= 0).mean())
            assert 0.15 < frac < 0.5, frac                                   # the scene's rejected share
            for name, sel in (("scene+constant+serpentine", slice(0, 3)), ("checker+zeros+corners", slice(3, 6))):
                o, m, c = _run_and_compare(eng, maps[sel], params, rng, f"{w}x{h} {params} n=3 {name}")
                seen |= set(np.unique(m).tolist())
                if sel.start == 0 and mx:
                    assert placed and {s for s, _, _ in placed} >= {1, mx, mx + 1}
                    for size, y0, x0 in placed:                              # the speckles are what decides at the threshold
                        assert (m[0, y0, x0] & dispfilter.SPECKLE != 0) == (size <= mx), (size, y0, x0)
                    assert c[1, 1] == 0 and c[1, 0] == w * h                 # the constant map: one component of H*W pixels
                    assert c[2, 1] == 0                                      # the serpentine is one component too
                if sel.start == 3 and mx:
                    assert c[0, 1] == (w * h + 1) // 2 and c[0, 0] == 0      # the checkerboard: every pixel its own component
                    assert c[1].tolist() == [0, 0, 0]
            o1, m1, _ = _run_and_compare(eng, maps[0], params, rng, f"{w}x{h} {params} n=1 (2-D)")
            assert o1.shape == (h, w) and m1.shape == (h, w)
            if small:                                                        # 9 maps: past the scratch's slice of 8
                nine = np.concatenate([maps, maps[:3, ::-1, ::-1]])
                _run_and_compare(eng, np.ascontiguousarray(nine), params, rng, f"{w}x{h} {params} n=9")
        assert seen == {0, 1, 16, 33, 48}                                    # the maps reach every class


@pytest.mark.gpu
def test_filter_device_mode_in_place_partial_outputs_and_determinism(model_factory):
    import torch
    w, h, n = 1280, 720, 3
    params = (40, 0.5, 16)
    maps, _ = _maps(w, h, 40, 5)
    maps = np.ascontiguousarray(maps[[0, 5, 2]])
    rng = np.random.default_rng(9)
    disp0 = rng.integers(0, 2 ** 32, maps.shape, dtype=np.uint32).view(np.float32)
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=n) as eng:
        want = dispfilter.reference(maps, *params, out_scale=eng.out_scale)
        d_raw = torch.from_numpy(maps).cuda()
        d_out = torch.zeros_like(d_raw)
        d_mask = torch.zeros(maps.shape, dtype=torch.uint8, device="cuda")
        d_disp = torch.from_numpy(disp0.copy()).cuda()
        d_cnt = torch.full((n, 3), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s1 = torch.cuda.Stream()
        eng.filter_raw_device(n, d_raw.data_ptr(), *params, out_raw_ptr=d_out.data_ptr(), mask_ptr=d_mask.data_ptr(),
                              disp_ptr=d_disp.data_ptr(), counts_ptr=d_cnt.data_ptr(), stream=s1.cuda_stream)
        s1.synchronize()
        assert np.array_equal(d_raw.cpu().numpy(), maps)                     # the input is only read
        assert np.array_equal(d_out.cpu().numpy(), want[0]) and np.array_equal(d_mask.cpu().numpy(), want[1])
        assert np.array_equal(d_cnt.cpu().numpy().view(np.uint32), want[2])
        assert np.array_equal(_bits(d_disp.cpu().numpy()), _expected_disp(disp0, want[0], want[1]))
        first = (d_out.cpu().numpy().tobytes(), d_mask.cpu().numpy().tobytes(), d_cnt.cpu().numpy().tobytes())
        # the same input again, on the filter's own stream (returns after completion): byte-identical
        d_out.zero_(), d_mask.zero_(), d_cnt.zero_()
        torch.cuda.synchronize()
        eng.filter_raw_device(n, d_raw.data_ptr(), *params, out_raw_ptr=d_out.data_ptr(), mask_ptr=d_mask.data_ptr(),
                              counts_ptr=d_cnt.data_ptr())
        assert first == (d_out.cpu().numpy().tobytes(), d_mask.cpu().numpy().tobytes(), d_cnt.cpu().numpy().tobytes())
        # mask only, with the counts; then out_raw only
        d_mask.zero_(), d_cnt.fill_(-1), d_out.fill_(-3)
        torch.cuda.synchronize()
        eng.filter_raw_device(n, d_raw.data_ptr(), *params, mask_ptr=d_mask.data_ptr(), counts_ptr=d_cnt.data_ptr(),
                              stream=s1.cuda_stream)
        s1.synchronize()
        assert np.array_equal(d_mask.cpu().numpy(), want[1]) and np.array_equal(d_cnt.cpu().numpy().view(np.uint32), want[2])
        assert np.all(d_out.cpu().numpy() == -3)
        eng.filter_raw_device(n, d_raw.data_ptr(), *params, out_raw_ptr=d_out.data_ptr(), stream=s1.cuda_stream)
        s1.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), want[0])
        # in place: out_raw == raw, on the caller's stream, both stages and then the fill alone on an unaligned view
        eng.filter_raw_device(n, d_raw.data_ptr(), *params, out_raw_ptr=d_raw.data_ptr(), mask_ptr=d_mask.data_ptr(),
                              stream=s1.cuda_stream)
        s1.synchronize()
        assert np.array_equal(d_raw.cpu().numpy(), want[0]) and np.array_equal(d_mask.cpu().numpy(), want[1])
        want_fill = dispfilter.reference(maps[:2], 0, 1.0, 25, out_scale=eng.out_scale)
        pad = torch.zeros(2 * h * w + 4, dtype=torch.int32, device="cuda")
        mpad = torch.zeros(2 * h * w + 4, dtype=torch.uint8, device="cuda")
        pad[1:1 + 2 * h * w] = torch.from_numpy(maps[:2]).cuda().reshape(-1)
        torch.cuda.synchronize()
        eng.filter_raw_device(2, pad.data_ptr() + 4, 0, 1.0, 25, out_raw_ptr=pad.data_ptr() + 4, mask_ptr=mpad.data_ptr() + 1,
                              stream=s1.cuda_stream)
        s1.synchronize()
        assert np.array_equal(pad.cpu().numpy()[1:1 + 2 * h * w].reshape(2, h, w), want_fill[0])
        assert np.array_equal(mpad.cpu().numpy()[1:1 + 2 * h * w].reshape(2, h, w), want_fill[1])
        assert pad[0].item() == 0 and not pad[1 + 2 * h * w:].any().item() and mpad[0].item() == 0 and not mpad[1 + 2 * h * w:].any().item()


@pytest.mark.gpu
def test_filter_argument_errors_leave_the_handle_usable(model_factory):
    w, h = 96, 64
    x = np.stack([synth.model_input_i8(w, h, D[(w, h)], 60 + k) for k in range(2)])
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=2, precision=api.PREC_F16) as eng:
        before = eng.infer(x)
        lib, hd = eng._lib, eng._h
        buf = np.ones((4, h, w), np.int32)                    # raw = buf[:2], out = buf[2:]: one allocation, to build overlaps
        raw, out = buf[:2], buf[2:]
        mask = np.empty((2, h, w), np.uint8)
        dsp = np.zeros((2, h, w), np.float32)
        cnt = np.zeros((2, 3), np.uint32)
        ok = api.SnFilterParams(5, 1.0, 4)

        def call(n=1, r=raw, p=ok, o=out, m=None, d=None, c=None, mem=api.SN_MEM_HOST):
            ptr = lambda a: a if isinstance(a, int) else api._np_ptr(a)      # noqa: E731
            return lib.sn_filter_raw(hd, n, ptr(r), C.byref(p) if p is not None else None, ptr(o), ptr(d), ptr(m), ptr(c),
                                     mem, None)

        def failed(rc):
            return rc == -1 and "sn_filter_raw" in lib.sn_last_error(hd).decode()

        assert call() == 0 and call(n=2, o=None, m=mask, c=cnt) == 0 and call(n=2, m=mask, d=dsp, c=cnt) == 0
        assert call(n=2, o=raw) == 0                                         # in place is allowed
        raw[:] = 1
        for n in (0, -1, 3):
            assert failed(call(n=n))
        assert failed(call(p=None)) and failed(call(r=None)) and failed(call(o=None, m=None)) and failed(call(mem=2))
        for p in (api.SnFilterParams(-1, 1.0, 4), api.SnFilterParams(w * h + 1, 1.0, 0), api.SnFilterParams(5, -0.5, 0),
                  api.SnFilterParams(5, float("nan"), 0), api.SnFilterParams(5, float("inf"), 0), api.SnFilterParams(5, 1.0, -1),
                  api.SnFilterParams(0, 1.0, 0)):
            assert failed(call(p=p)), (p.speckle_max_px, p.speckle_diff_px, p.fill_max_px)
        assert call(p=api.SnFilterParams(w * h, 0.0, 0)) == 0                # the bounds themselves are allowed
        assert call(p=api.SnFilterParams(0, float("nan"), 0)) == -1
        # any overlap but out_raw == raw
        assert failed(call(n=2, o=raw.ctypes.data + 4 * h * w))              # out_raw inside raw, shifted by a map
        assert failed(call(n=1, o=None, m=raw.view(np.uint8))) and failed(call(n=1, d=raw.view(np.float32)))
        assert failed(call(n=1, d=out.view(np.float32))) and failed(call(n=1, c=out.view(np.uint32)))
        assert failed(call(n=1, m=mask, c=mask.view(np.uint32)))
        assert "overlap" in lib.sn_last_error(hd).decode()
        with pytest.raises(api.StereoNetError):
            eng.filter_raw(raw[:, :-1], 5, 1.0, 4)
        with pytest.raises(api.StereoNetError):
            eng.filter_raw(raw, 5, 1.0, 4, disp=np.zeros((2, h, w), np.float64))
        with pytest.raises(api.StereoNetError):
            eng.filter_raw(np.ones((3, h, w), np.int32), 5, 1.0, 4)
        after = eng.infer(x)                                                 # existing calls are unchanged by all of this
        assert np.array_equal(after[1], before[1]) and np.array_equal(_bits(after[0]), _bits(before[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1280, 720), (96, 64)])
def test_filter_composes_with_lrc_point_cloud_and_depth(model_factory, w, h):
    n = 2
    x = np.stack([synth.model_input_i8(w, h, D[(w, h)], 80 + k) for k in range(n)])
    params = (200, 1.0, 16)
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=n, precision=api.PREC_F16) as eng:
        plain_before = eng.infer(x)                                          # sn_infer_batch
        disp, raw, lmask, kept = eng.infer_lrc(x, 1.0, 0.0)
        fdisp = disp.copy()
        out, mask, counts = eng.filter_raw(raw, *params, disp=fdisp)
        w_out, w_mask, w_counts = dispfilter.reference(raw, *params, out_scale=eng.out_scale)
        print(f"{w}x{h}: kept {kept.tolist()}, after the filter {counts.tolist()}")
        assert np.array_equal(out, w_out) and np.array_equal(mask, w_mask) and np.array_equal(counts, w_counts)
        assert np.array_equal(_bits(fdisp), _expected_disp(disp, w_out, w_mask))
        assert np.array_equal(mask & dispfilter.INVALID_IN != 0, lmask != 0)   # invalid in = rejected by the check (1, or 33 once filled)
        assert np.array_equal(counts[:, 0], kept - counts[:, 1] + counts[:, 2])
        _, pc_counts = eng.pointcloud(out, pointcloud.Camera(), pointcloud.COMPACT)
        assert np.array_equal(pc_counts, counts[:, 0])
        depth = eng.depth_from_raw(out)
        assert np.array_equal(np.isfinite(depth), out > 0)
        plain_after = eng.infer(x)
        for a, b in zip(plain_before, plain_after):                          # existing calls: identical bytes around a filter call
            assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_filelist_speckle_and_fill(model_factory, tmp_path, capsys):
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
    assert filelist.main(base + ["--out", str(tmp_path / "flt"), "--gt", str(tmp_path / "gt.list"), "--lrc", "1",
                                 "--speckle", "200,1", "--fill", "16"]) == 0
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert sorted(os.listdir(tmp_path / "flt")) == sorted(
        f"{i}.{e}" for i in (0, 1) for e in ("raw.bin", "disp.pfm", "depth.ppm", "mask.pgm", "filter.pgm"))
    removed = filled = 0
    densities = []
    gt = synth.disparity_field(w, h, d)
    with api.StereoNetHIP(model, precision=api.PREC_F16) as eng:
        recs = filelist.run_imglist(eng, str(tmp_path / "l.list"), str(tmp_path / "r.list"), gt_list=str(tmp_path / "gt.list"),
                                    lrc=(1.0, 0.0), flt=(200, 1.0, 16))
        for i in range(2):
            eyes = [images.bgr_to_nv12(images.imread_bgr(names[s][i])) for s in ("l", "r")]
            sbs = images.sbs_from_eyes(eyes[0], eyes[1], w, h)
            mdisp, mraw, lmask, kept = eng.infer_lrc(sbs, 1.0, 0.0)
            w_out, w_mask, w_counts = dispfilter.reference(mraw, 200, 1.0, 16, out_scale=eng.out_scale)
            rd = lambda p: open(p, "rb").read()      # noqa: E731
            assert rd(tmp_path / "flt" / f"{i}.raw.bin") == w_out.tobytes()
            assert np.array_equal(images.read_pnm(str(tmp_path / "flt" / f"{i}.filter.pgm")), w_mask)
            assert np.array_equal(images.read_pnm(str(tmp_path / "flt" / f"{i}.mask.pgm")), lmask)
            assert np.array_equal(_bits(images.read_pfm(str(tmp_path / "flt" / f"{i}.disp.pfm"))),
                                  _expected_disp(mdisp, w_out, w_mask))
            rec = recs[i]
            assert np.array_equal(rec["raw"], w_out) and np.array_equal(rec["filter_mask"], w_mask)
            assert (rec["removed"], rec["filled"]) == (int(w_counts[0, 1]), int(w_counts[0, 2]))
            assert rec["density"] == float(w_counts[0, 0]) / (w * h) == float((w_out > 0).sum()) / (w * h)
            assert rec["metrics"]["valid_px"] == int(((w_mask == 0) & (gt < d)).sum())
            assert rec["metrics_filled"]["valid_px"] == int(((w_mask & 32 != 0) & (gt < d)).sum())
            removed += rec["removed"]
            filled += rec["filled"]
            densities.append(rec["density"])
    assert set(summary) == {"frames", "epe", "bad1", "bad3", "d1", "filled_epe", "removed", "filled", "density"}
    assert summary["frames"] == 2 and summary["removed"] == removed and summary["filled"] == filled
    assert summary["density"] == pytest.approx(np.mean(densities), abs=1e-12)
