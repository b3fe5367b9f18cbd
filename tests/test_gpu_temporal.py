"""sn_temporal_push on the MI355X: the kernel equals the numpy twin (hobot_stereonet_amd/temporal.py) at every pixel — out, mask,
counts and the float map's bits — on the 12-frame clip of temporal.noisy_sequence, for four settings, both guide forms, NV12
at pitch W and 2W, host and device buffers; the state carries across calls (12 = 12 x 1 = 5 + 7), streams interleaved in one
call equal separate filters, in place, reset, determinism, argument errors, the composition with the rest of the chain, the
file-list harness's --temporal and the node (STEREONET_TEMPORAL).  The twin's answers are computed once per (shape, setting).

tests/test_temporal.py asserts that the clip's masks hold every value a setting can produce; it is asserted again here, so
that the comparison cannot pass on an idle filter."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from hobot_stereonet_amd import api, dispfilter, lrcheck, smooth, synth, temporal

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
D = {(96, 64): 48, (1242, 375): 256}
T = 12
# (alpha, q, persist, luma_delta): q = delta_px in raw units; the issue's four settings and the mask values each must produce
SETTINGS = {(64, 1000, 2, 24): {0, 1, 2, 5, 8, 9, 16}, (256, 0, 1, 0): {0, 1, 5, 16},
            (128, 400, 0, 24): {0, 1, 2, 8, 9, 16}, (64, 1000, 8, 0): {0, 1, 2, 5, 16}}
CASES = [(w, h, s) for (w, h) in D for s in SETTINGS]


def _params(setting):
    a, q, p, l = setting
    return (a, temporal.delta_for(q), p, l)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _clip(w, h):
    raw, luma, _ = temporal.noisy_sequence(w, h, T, w + h)
    raw.setflags(write=False)
    luma.setflags(write=False)
    return raw, luma


@functools.lru_cache(maxsize=None)
def _want(w, h, setting):
    raw, luma = _clip(w, h)
    got = temporal.reference(raw, luma, _params(setting))
    for a in got:
        a.setflags(write=False)
    return got


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


def _check(tag, got, want, raw=None, disp=None, disp0=None, sel=slice(None)):
    out, mask, counts = got
    w_out, w_mask, w_counts = (a[sel] for a in want)
    print(f"{tag}: counts {counts.sum(0).tolist()}, differing pixels (out, mask) = {int((out != w_out).sum())}, "
          f"{int((mask != w_mask).sum())}")
    assert np.array_equal(mask, w_mask), tag
    assert np.array_equal(out, w_out), tag
    assert np.array_equal(counts, w_counts), tag
    if disp is not None:                                             # untouched words keep their random bit pattern
        assert np.array_equal(_bits(disp), _bits(temporal.expected_disp(disp0, raw[sel], w_out))), tag


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,setting", CASES, ids=[f"{w}x{h}-a{s[0]}-q{s[1]}-p{s[2]}-l{s[3]}" for w, h, s in CASES])
def test_temporal_kernel_equals_twin_bit_for_bit(model_factory, w, h, setting):
    import torch
    raw, luma = _clip(w, h)
    want = _want(w, h, setting)
    values = dict(zip(*[a.tolist() for a in np.unique(want[1], return_counts=True)]))
    print(f"{w}x{h} {setting}: mask values {values}")
    assert set(values) == SETTINGS[setting]
    rng = np.random.default_rng(w + h + setting[0])
    disp0 = rng.integers(0, 2 ** 32, raw.shape, dtype=np.uint32).view(np.float32)
    hw = h * w
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=T) as eng, eng.temporal_filter(1, *_params(setting)) as tf:
        results = []
        for kind, guide, pitch in ((api.SN_GUIDE_NV12, _nv12(luma, w), w), (api.SN_GUIDE_NV12, _nv12(luma, 2 * w), 2 * w),
                                   (api.SN_GUIDE_TENSOR, _tensor(luma), 0)):
            disp = disp0.copy()
            tf.reset()
            got = tf.push(raw, guide, kind, pitch, disp=disp)
            _check(f"host, guide kind {kind} pitch {pitch}", got, want, raw, disp, disp0)
            results.append(b"".join(a.tobytes() for a in got) + disp.tobytes())
        assert results[0] == results[1] == results[2]
        # device buffers on a caller's stream: aligned buffers and the tensor guide (the vectorised form where W % 4 == 0),
        # then out one word, mask and NV12 guide (pitch 2W) one byte off 16-byte alignment (the scalar form at every width);
        # four guard words around every output
        s1 = torch.cuda.Stream()
        for odd in (0, 1):
            d_raw = torch.from_numpy(raw.copy()).cuda()
            host_guide = _nv12(luma, 2 * w) if odd else _tensor(luma).reshape(-1).view(np.uint8)
            d_guide = torch.zeros(host_guide.size + 1, dtype=torch.uint8, device="cuda")
            d_guide[odd:odd + host_guide.size].copy_(torch.from_numpy(host_guide))
            go, gm = (1, 1) if odd else (4, 4)                                   # guard elements in front of out and mask
            d_out = torch.full((T * hw + 8,), -3, dtype=torch.int32, device="cuda")
            d_mask = torch.full((T * hw + 8,), 77, dtype=torch.uint8, device="cuda")
            d_disp = torch.from_numpy(disp0.copy()).cuda()
            d_cnt = torch.full((T, 4), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            tf.reset(0)
            tf.push_device(T, d_raw.data_ptr(), d_guide.data_ptr() + odd, api.SN_GUIDE_NV12 if odd else api.SN_GUIDE_TENSOR,
                           2 * w if odd else 0, out_raw_ptr=d_out.data_ptr() + 4 * go, mask_ptr=d_mask.data_ptr() + gm,
                           disp_ptr=d_disp.data_ptr(), counts_ptr=d_cnt.data_ptr(), stream=s1.cuda_stream)
            s1.synchronize()
            o, m = d_out.cpu().numpy(), d_mask.cpu().numpy()
            assert np.all(o[:go] == -3) and np.all(o[go + T * hw:] == -3)        # the guard words around the outputs
            assert np.all(m[:gm] == 77) and np.all(m[gm + T * hw:] == 77)
            assert np.array_equal(d_raw.cpu().numpy(), raw)                      # the input is only read
            dev = (o[go:go + T * hw].reshape(raw.shape), m[gm:gm + T * hw].reshape(raw.shape), d_cnt.cpu().numpy().view(np.uint32))
            _check(f"device, odd offsets {odd}", dev, want, raw, d_disp.cpu().numpy(), disp0)


@pytest.mark.gpu
def test_temporal_state_carries_across_calls_and_runs_are_identical(model_factory):
    w, h, setting = 96, 64, (64, 1000, 2, 24)
    raw, luma = _clip(w, h)
    want = _want(w, h, setting)
    guide = _tensor(luma)
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=T) as eng, eng.temporal_filter(1, *_params(setting)) as tf:
        whole = tf.push(raw, guide, api.SN_GUIDE_TENSOR)
        _check("12 in one push", whole, want)
        tf.reset()
        again = tf.push(raw, guide, api.SN_GUIDE_TENSOR)                         # two runs give identical bits
        assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, again))
        tf.reset()
        ones = [tf.push(raw[k], guide[k], api.SN_GUIDE_TENSOR) for k in range(T)]
        assert ones[0][0].shape == (h, w) and ones[0][2].shape == (1, 4)
        singles = (np.stack([o[0] for o in ones]), np.stack([o[1] for o in ones]), np.concatenate([o[2] for o in ones]))
        _check("12 pushes of 1", singles, want)
        tf.reset(0)
        a, b = tf.push(raw[:5], guide[:5], api.SN_GUIDE_TENSOR), tf.push(raw[5:], guide[5:], api.SN_GUIDE_TENSOR)
        _check("5 + 7", tuple(np.concatenate([x, y]) for x, y in zip(a, b)), want)
        # without a reset the stream goes on: the clip a second time is frames 13..24 of one stream
        twice = temporal.reference(np.concatenate([raw, raw]), np.concatenate([luma, luma]), _params(setting))
        tf.reset()
        tf.push(raw, guide, api.SN_GUIDE_TENSOR)
        _check("frames 13..24", tf.push(raw, guide, api.SN_GUIDE_TENSOR), twice, sel=slice(T, 2 * T))
        assert not np.array_equal(twice[1][T], want[1][0])


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", list(D))
def test_temporal_streams_interleaved_in_place_and_reset(model_factory, w, h):
    import torch
    setting = (64, 1000, 2, 24)
    raw, luma = _clip(w, h)
    # three clips of four frames: frames 0..3, 4..7 and 8..11 of the sequence, interleaved a b c a b c ... in one call
    order = [4 * s + f for f in range(4) for s in range(3)]
    ids = [s for f in range(4) for s in range(3)]
    iraw, iluma = np.ascontiguousarray(raw[order]), np.ascontiguousarray(luma[order])
    want = temporal.reference(iraw, iluma, _params(setting), ids)
    per = [temporal.reference(raw[4 * s:4 * s + 4], luma[4 * s:4 * s + 4], _params(setting)) for s in range(3)]
    for j, k in enumerate(order):                                                # the twin itself: interleaved == per clip
        assert np.array_equal(want[0][j], per[k // 4][0][k % 4]) and np.array_equal(want[1][j], per[k // 4][1][k % 4])
    guide = _nv12(iluma, 2 * w)
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=T) as eng:
        with eng.temporal_filter(3, *_params(setting)) as tf:
            got = tf.push(iraw, guide, api.SN_GUIDE_NV12, 2 * w, stream_of=ids)
            _check("3 streams in one call", got, want)
            for s in range(3):                                                   # ... equal three separate filters
                with eng.temporal_filter(1, *_params(setting)) as one:
                    sel = [j for j in range(T) if ids[j] == s]
                    alone = one.push(iraw[sel], _nv12(iluma[sel], w), api.SN_GUIDE_NV12, w)
                    assert all(np.array_equal(a, b[sel]) for a, b in zip(alone, got)), s
            # reset of stream 1 leaves 0 and 2 alone: the next call continues their clips and restarts stream 1's
            tf.reset(1)
            states = {}
            temporal.reference(iraw, iluma, _params(setting), ids, states)
            del states[1]
            more = temporal.reference(iraw[:6], iluma[:6], _params(setting), ids[:6], states)
            _check("after reset(1)", tf.push(iraw[:6], guide, api.SN_GUIDE_NV12, 2 * w, stream_of=ids[:6]), more)
            assert not np.array_equal(more[1][0], want[1][0]) and np.array_equal(more[1][1], want[1][1])
            # in place on the device (out_raw == raw), all three streams, the filter's own stream
            tf.reset()
            pad = torch.full((T * h * w + 8,), -3, dtype=torch.int32, device="cuda")
            d_raw = pad[4:4 + T * h * w]
            d_raw.copy_(torch.from_numpy(iraw).reshape(-1))
            d_guide = torch.from_numpy(guide).cuda()
            d_mask = torch.zeros(T * h * w, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            tf.push_device(T, d_raw.data_ptr(), d_guide.data_ptr(), api.SN_GUIDE_NV12, 2 * w, stream_of=ids,
                           out_raw_ptr=d_raw.data_ptr(), mask_ptr=d_mask.data_ptr())
            assert np.array_equal(d_raw.cpu().numpy().reshape(iraw.shape), want[0])
            assert np.array_equal(d_mask.cpu().numpy().reshape(iraw.shape), want[1])
            assert np.all(pad[:4].cpu().numpy() == -3) and np.all(pad[4 + T * h * w:].cpu().numpy() == -3)
            # host mode with out == raw is the same call through the staging
            tf.reset()
            inplace, sid = iraw.copy(), np.array(ids, np.int32)
            assert eng._lib.sn_temporal_push(tf._t, T, sid.ctypes.data, inplace.ctypes.data, guide.ctypes.data, api.SN_GUIDE_NV12,
                                             2 * w, inplace.ctypes.data, None, None, None, api.SN_MEM_HOST, None) == 0
            assert np.array_equal(inplace, want[0])


@pytest.mark.gpu
def test_temporal_argument_errors_and_destroy_order(model_factory):
    w, h = 96, 64
    x = np.stack([synth.model_input_i8(w, h, D[(w, h)], 60 + k) for k in range(2)])
    eng = api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=2, precision=api.PREC_F16)
    lib, hd = eng._lib, eng._h
    before = eng.infer(x)

    def failed(rc, name):
        return rc == -1 and name in lib.sn_last_error(hd).decode()

    t = C.c_void_p()
    ok = api.SnTemporalParams(64, 0.5, 2, 24)
    bad = [lib.sn_temporal_create(hd, n, C.byref(ok), C.byref(t)) for n in (0, -1, 3)]
    bad += [lib.sn_temporal_create(hd, 1, None, C.byref(t)), lib.sn_temporal_create(hd, 1, C.byref(ok), None)]
    for prm in ((0, 0.5, 2, 24), (257, 0.5, 2, 24), (64, -0.5, 2, 24), (64, float("nan"), 2, 24), (64, float("inf"), 2, 24),
                (64, 0.5, -1, 24), (64, 0.5, 9, 24), (64, 0.5, 2, -1), (64, 0.5, 2, 256)):
        bad.append(lib.sn_temporal_create(hd, 1, C.byref(api.SnTemporalParams(*prm)), C.byref(t)))
    assert all(failed(rc, "sn_temporal_create") for rc in bad) and not t.value, bad
    for prm in ((1, 0.0, 0, 0), (256, 3.0e38, 8, 255)):                        # the bounds themselves are allowed
        with eng.temporal_filter(2, *prm):
            pass
    tf = eng.temporal_filter(2, 64, 0.5, 2, 24)
    buf = np.ones((4, h, w), np.int32)                        # raw = buf[:2], out = buf[2:]: one allocation, to build overlaps
    raw, out = buf[:2], buf[2:]
    out[:] = -5
    mask = np.full((2, h, w), 99, np.uint8)
    dsp = np.full((2, h, w), 7.0, np.float32)
    cnt = np.full((2, 4), 12345, np.uint32)
    nv = np.zeros(2 * (h + h // 2) * 2 * w + 2 * h * w * 4, np.uint8)
    ten = np.zeros((2, 6, h, w), np.int8)
    ids = np.zeros(2, np.int32)

    def call(n=1, sid=None, r=raw, g=nv, kind=api.SN_GUIDE_NV12, pitch=w, o=out, m=None, d=None, c=None, mem=api.SN_MEM_HOST, f=None):
        ptr = lambda a: a if isinstance(a, int) or a is None else a.ctypes.data      # noqa: E731
        return lib.sn_temporal_push((f or tf)._t, n, ptr(sid), ptr(r), ptr(g), kind, pitch, ptr(o), ptr(d), ptr(m), ptr(c), mem, None)

    bad = [call(n=n, m=mask, d=dsp, c=cnt) for n in (0, -1, 3)]
    bad += [call(r=None), call(o=None, m=None), call(mem=2), call(g=None), call(g=None, kind=api.SN_GUIDE_TENSOR)]
    bad += [call(kind=2), call(kind=-1), call(pitch=w - 2), call(pitch=w + 1), call(pitch=0), call(pitch=-w)]
    bad += [call(n=2, sid=np.array([0, 2], np.int32)), call(n=2, sid=np.array([-1, 0], np.int32))]
    assert all(failed(rc, "sn_temporal_push") for rc in bad), bad
    over = [call(n=2, o=raw.ctypes.data + 4 * h * w), call(o=None, m=raw.view(np.uint8)), call(d=raw.view(np.float32)),
            call(d=out.view(np.float32)), call(c=out.view(np.uint32)), call(m=mask, c=mask.view(np.uint32)),
            call(m=mask, d=dsp, c=dsp.view(np.uint32)), call(g=out.view(np.uint8)), call(o=None, m=nv),
            call(n=2, g=ten, kind=api.SN_GUIDE_TENSOR, o=None, m=ten.view(np.uint8).reshape(-1)[6 * h * w:]),
            call(g=raw.view(np.uint8), o=raw)]
    assert all(failed(rc, "sn_temporal_push") for rc in over), over
    assert "overlap" in lib.sn_last_error(hd).decode()
    assert failed(lib.sn_temporal_reset(tf._t, 2), "sn_temporal_reset") and failed(lib.sn_temporal_reset(tf._t, -2), "sn_temporal_reset")
    # nothing was written by any failed call, and none of them touched the state: the first good push is a first frame
    assert np.all(out == -5) and np.all(raw == 1) and np.all(mask == 99) and np.all(dsp == 7.0) and np.all(cnt == 12345)
    assert call(m=mask, c=cnt) == 0 and np.all(mask[0] == 0) and np.all(out[0] == 1) and cnt[0].tolist() == [h * w, 0, 0, 0]
    assert call(n=2, sid=ids, o=raw) == 0 and call(n=2, sid=np.array([1, 0], np.int32), g=ten, kind=api.SN_GUIDE_TENSOR, pitch=-1) == 0
    assert call(pitch=2 * w) == 0 and call(n=2, g=raw.view(np.uint8), o=out) == 0
    with eng.temporal_filter(1, 64, 0.5, 2, 0) as plain:                         # luma_delta == 0 reads no guide: none, or any kind
        assert call(g=None, f=plain) == 0 and call(g=None, kind=7, pitch=0, f=plain) == -1 and call(g=None, pitch=0, f=plain) == 0
    with pytest.raises(api.StereoNetError):
        tf.push(raw[:, :-1], nv)
    with pytest.raises(api.StereoNetError):
        tf.push(raw, nv, stream_of=[0])
    with pytest.raises(api.StereoNetError):
        tf.push(raw, np.zeros(h * w, np.uint8))                                  # two maps, one frame of luma
    after = eng.infer(x)                                                         # existing calls are unchanged by all of this
    assert np.array_equal(after[1], before[1]) and np.array_equal(_bits(after[0]), _bits(before[0]))
    # destroying the handle under a live filter is refused and leaves both usable
    assert lib.sn_destroy(hd) == -6 and "temporal" in lib.sn_last_error(hd).decode()
    with pytest.raises(api.StereoNetError):
        eng.close()
    assert call(m=mask) == 0 and np.array_equal(eng.infer(x)[1], before[1])
    tf.close()
    eng.close()
    assert not eng._h.value


@pytest.mark.gpu
def test_temporal_composes_with_the_rest_of_the_chain(model_factory):
    w, h, n = 96, 64, 4
    setting = (64, 25.0, 2, 24)              # a wide delta_px: the frames' maps differ by whatever the network makes of the noise
    # a 4-frame synthetic clip: one scene with sensor noise of its own in every frame and a patch that moves down the image
    rng = np.random.default_rng(80)
    base = synth.model_input_i8(w, h, D[(w, h)], 80).astype(np.int16)
    x = np.stack([np.clip(base + rng.integers(-3, 4, base.shape), -128, 127).astype(np.int8) for _ in range(n)])
    for k in range(n):
        x[k, :, 8 * k:8 * k + 8, 10:40] ^= np.int8(0x55)
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=n, precision=api.PREC_F16) as eng:
        disp, raw, lmask, kept = eng.infer_lrc(x, 1.0, 0.0)
        fout, fmask, _ = eng.filter_raw(raw, 200, 1.0, 16, disp=disp)
        sout, smask, _ = eng.smooth_raw(fout, x, api.SN_GUIDE_TENSOR, 0, 2, 12, 5, disp=disp)
        with eng.temporal_filter(1, *setting) as tf:
            tdisp = disp.copy()
            out, tmask, counts = tf.push(sout, x, api.SN_GUIDE_TENSOR, disp=tdisp)
        depth = eng.depth_from_raw(out)
        # the same composition of twins, from the two forward passes on
        _, left = eng.infer(x)
        _, mirrored = eng.infer(eng.mirror_pair(x))
        scale = eng.out_scale
    t_l, t_lmask, _ = lrcheck.reference(left, mirrored, 1.0, 0.0, True, out_scale=scale)
    t_f, t_fmask, _ = dispfilter.reference(t_l, 200, 1.0, 16, out_scale=scale)
    luma = smooth.luma_from_tensor(x)
    t_s, t_smask, _ = smooth.reference(t_f, luma, 2, 12, 5, out_scale=scale)
    t_out, t_tmask, t_counts = temporal.reference(t_s, luma, setting, out_scale=scale)
    print(f"kept {kept.tolist()}, temporal counts {counts.tolist()}, mask values {np.unique(tmask).tolist()}")
    assert np.array_equal(lmask, t_lmask) and np.array_equal(fmask, t_fmask) and np.array_equal(smask, t_smask)
    assert np.array_equal(out, t_out) and np.array_equal(tmask, t_tmask) and np.array_equal(counts, t_counts)
    assert (tmask & temporal.BLENDED).any()
    assert np.array_equal(_bits(tdisp), _bits(temporal.expected_disp(disp, sout, out, scale)))
    f, B = np.float32(527.1931762695312), np.float32(119.89382172)
    with np.errstate(divide="ignore"):
        dis = t_out.astype(np.float32) * np.float32(scale)
        ref = (np.float64(f * B) / (dis.astype(np.float64) * 16.0 * 12.0) / 1000.0).astype(np.float32)
    assert np.array_equal(depth, ref) and np.array_equal(np.isfinite(depth), out > 0)


def _write_lists(tmp_path, w, h, d, n):
    from hobot_stereonet_amd import images
    names = {"l": [], "r": []}
    lt0, rt0 = synth.stereo_pair_u8(w, h, d, 70)
    rng = np.random.default_rng(70)
    for k in range(n):                                                   # one scene, noise of its own per frame: not a constant clip
        lt, rt = (np.clip(e.astype(np.int16) + rng.integers(-3, 4, e.shape), 0, 255).astype(np.uint8) for e in (lt0, rt0))
        for side, eye in (("l", lt), ("r", rt)):
            p = str(tmp_path / f"{side}{k}.png")
            images.write_png(p, np.ascontiguousarray(eye.transpose(1, 2, 0)))
            names[side].append(p)
    gts = []
    for k in range(n):
        p = str(tmp_path / f"gt{k}.pfm")
        images.write_pfm(p, synth.disparity_field(w, h, d))
        gts.append(p)
    for side, lst in (("l", names["l"]), ("r", names["r"]), ("gt", gts)):
        (tmp_path / f"{side}.list").write_text("".join(f"{p}\n" for p in lst))
    return names


@pytest.mark.gpu
def test_filelist_temporal(model_factory, tmp_path, capsys):
    from hobot_stereonet_amd import filelist, images
    w, h, d, n = 96, 64, 48, 4
    model = model_factory(w, h, d)
    names = _write_lists(tmp_path, w, h, d, n)
    base = ["--model", model, "--left", str(tmp_path / "l.list"), "--right", str(tmp_path / "r.list"), "--precision", "f16"]
    capsys.readouterr()
    assert filelist.main(base + ["--out", str(tmp_path / "o"), "--gt", str(tmp_path / "gt.list"), "--temporal", "64,25,2,24"]) == 0
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert sorted(os.listdir(tmp_path / "o")) == sorted(
        f"{i}.{e}" for i in range(n) for e in ("raw.bin", "disp.pfm", "depth.ppm", "temporal.pgm"))
    assert {"blended", "held", "density", "temporal_epe_before", "temporal_epe_after", "flicker_before", "flicker_after"} <= set(summary)
    assert summary["frames"] == n and summary["blended"] > 0
    print(summary)
    maps, lumas = [], []
    with api.StereoNetHIP(model, precision=api.PREC_F16) as eng:
        for i in range(n):
            eyes = [images.bgr_to_nv12(images.imread_bgr(names[s][i])) for s in ("l", "r")]
            sbs = images.sbs_from_eyes(eyes[0], eyes[1], w, h)
            maps.append(eng.infer_sbs_nv12(sbs)[1])
            lumas.append(smooth.luma_from_nv12(sbs, w, h, 2 * w)[0])
        scale = eng.out_scale
    w_out, w_mask, w_counts = temporal.reference(np.stack(maps), np.stack(lumas), (64, 25.0, 2, 24), out_scale=scale)
    for i in range(n):
        assert open(tmp_path / "o" / f"{i}.raw.bin", "rb").read() == w_out[i].tobytes()
        assert np.array_equal(images.read_pnm(str(tmp_path / "o" / f"{i}.temporal.pgm")), w_mask[i])
    assert summary["blended"] == int(w_counts[:, 1].sum()) and summary["held"] == int(w_counts[:, 2].sum())
    assert summary["density"] == pytest.approx(float(w_counts[:, 0].mean()) / (w * h), abs=1e-12)
    s = float(temporal.wire_scale(scale))
    assert summary["flicker_before"] == pytest.approx(temporal.flicker(np.stack(maps)) * s)
    assert summary["flicker_after"] == pytest.approx(temporal.flicker(w_out) * s)


def _payloads(prefix, n, w, h):
    return np.stack([np.fromfile(f"{prefix}.{i}.msg", np.int32, w * h).reshape(h, w) for i in range(n)])


@pytest.mark.gpu
def test_node_filters_the_disparity_stream(model_factory, tmp_path):
    subprocess.check_call(["make", "-C", COMPAT, "-s"])
    w, h, d, n = 96, 64, 48, 4
    m = model_factory(w, h, d)
    rng = np.random.default_rng(8)
    frames = []
    lt, rt = synth.stereo_pair_u8(w, h, d, 8)
    for k in range(n):                                                   # four DIFFERENT frames: noise per frame, a moving bright bar
        f = rng.integers(0, 256, (h * 3 // 2, 2 * w), dtype=np.uint8)
        f[:h, :w] = np.clip(lt[0].astype(np.int16) + rng.integers(-3, 4, (h, w)), 0, 255)
        f[:h, w:] = np.clip(rt[0].astype(np.int16) + rng.integers(-3, 4, (h, w)), 0, 255)
        f[10:20, 6 * k:6 * k + 12] = 250
        frames.append(f)
    sbs = np.stack(frames)
    sbs.tofile(str(tmp_path / "s.bin"))
    exe = os.path.join(COMPAT, "build", "temporal_harness")
    env = {k: v for k, v in os.environ.items() if not k.startswith("STEREONET_TEMPORAL")}
    env["STEREONET_PRECISION"] = "fp32"             # pinned: the default's first-call calibration is not a function of the frame
    args = [exe, m, str(tmp_path / "s.bin"), str(w), str(h), str(n)]
    off = subprocess.run(args + [str(tmp_path / "off")], capture_output=True, text=True, env=env, timeout=120)
    assert off.returncode == 0 and f"received={n}" in off.stdout, off.stderr[-2000:]
    setting = (64, 25.0, 2, 24)
    on = subprocess.run(args + [str(tmp_path / "on")], capture_output=True, text=True, timeout=120,
                        env=dict(env, STEREONET_TEMPORAL=",".join(str(v) for v in setting)))
    assert on.returncode == 0 and f"received={n}" in on.stdout, on.stderr[-2000:]
    assert "temporal filter:" in on.stderr and "temporal filter failed" not in on.stderr
    plain, filtered = _payloads(tmp_path / "off", n, w, h), _payloads(tmp_path / "on", n, w, h)
    assert len({p.tobytes() for p in plain}) == n                                # the clip is not constant
    luma = np.ascontiguousarray(sbs[:, :h, :w])
    want, mask, counts = temporal.reference(plain, luma, setting)
    print(f"node: temporal counts {counts.tolist()}, mask values {np.unique(mask).tolist()}")
    assert np.array_equal(filtered, want) and not np.array_equal(filtered, plain)
    assert (mask & temporal.BLENDED).any() and (mask & (temporal.MOVED | temporal.JUMP)).any()
    for i in range(n):                                                           # the JPEG behind the tensor is untouched
        a, b = open(f"{tmp_path / 'off'}.{i}.msg", "rb").read(), open(f"{tmp_path / 'on'}.{i}.msg", "rb").read()
        assert a[4 * w * h:] == b[4 * w * h:] and len(a) > 4 * w * h
    # a bad value turns the filter off with one error line; the payloads are the unfiltered ones
    bad = subprocess.run(args + [str(tmp_path / "bad")], capture_output=True, text=True, timeout=120,
                         env=dict(env, STEREONET_TEMPORAL="300,25"))
    assert bad.returncode == 0 and bad.stderr.count("no temporal filter") == 1, bad.stderr[-2000:]
    assert np.array_equal(_payloads(tmp_path / "bad", n, w, h), plain)


@pytest.mark.gpu
def test_node_request_without_a_frame(model_factory, tmp_path):
    """The offline feeder's requests carry no side-by-side frame.  With LUMA_DELTA > 0 there is no luma to compare: the map
    passes unfiltered (and the stream is reset); with LUMA_DELTA = 0 the filter needs no guide and filters them like any other."""
    subprocess.check_call(["make", "-C", COMPAT, "-s"])
    w, h, d, n = 96, 64, 48, 3
    m = model_factory(w, h, d)
    _write_lists(tmp_path, w, h, d, n)
    exe = os.path.join(COMPAT, "build", "stereonet_filelist")
    env = {k: v for k, v in os.environ.items() if not k.startswith("STEREONET_TEMPORAL")}
    env.update(STEREONET_PRECISION="fp32", STEREONET_FEED_PAUSE_MS="0")
    maps = {}
    for tag, value in (("off", None), ("guided", "64,25,2,24"), ("plain", "64,25,2")):
        os.makedirs(tmp_path / tag)
        r = subprocess.run([exe, m, str(tmp_path / "l.list"), str(tmp_path / "r.list"), str(tmp_path / tag)], capture_output=True,
                           text=True, timeout=120, env=env if value is None else dict(env, STEREONET_TEMPORAL=value))
        assert r.returncode == 0 and f"fed={n} received={n}" in r.stdout, r.stderr[-2000:]
        assert r.stderr.count("map not filtered") == (1 if tag == "guided" else 0) and "temporal filter failed" not in r.stderr
        maps[tag] = np.stack([np.fromfile(str(tmp_path / tag / f"{i}.raw.bin"), np.int32).reshape(h, w) for i in range(n)])
    assert np.array_equal(maps["guided"], maps["off"])
    want, mask, _ = temporal.reference(maps["off"], None, (64, 25.0, 2, 0))
    assert np.array_equal(maps["plain"], want) and (mask & temporal.BLENDED).any()
