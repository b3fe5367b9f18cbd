"""Every post-processing stage on the MI355X at the geometries of tests/golden/postproc_domain.py: maps narrower than a wave or a
vector, one-row and one-column maps, tile and segment remainders of exactly one, and sample counts of one below, exactly and one
above a compact tile.  One handle per geometry; for every stage and setting the result equals the numpy twin bit for bit (maps,
masks, counts, point records, the float maps' bits) in host mode and in device mode on a caller's stream, the device run once with
16-byte aligned buffers and once with the outputs, the masks and the NV12 guide one element or byte off alignment (both kernel
forms run wherever the width permits the vector one), 0x5a guard bytes around every output, the inputs read back unchanged.  The
calls the header refuses (postproc_domain.REFUSALS) return SN_ERR_ARG, write nothing and leave the handle usable.
tests/test_postproc_domain.py checks on the CPU that the twins are right at these geometries and that the inputs exercise every
mask value; the union of the mask values the GPU produced is asserted again here.

The slice walks of sn_temporal_push and sn_costmap_push (64 maps per launch) run at the end: pushes of 130 and 70 maps on three
streams, so that the second and third launch of a call execute with `fresh`, the previous origin and the moved pointers."""
import os
import time

import numpy as np
import pytest

import postproc_domain as dom
from hobot_stereonet_amd import api, costmap, obstacles, pointcloud, rectify, render, smooth, temporal

GUARD = 16
FILL = 0x5a
N = dom.N
GEOMS = list(dom.GEOMETRIES)
_seen = {}            # (stage, setting) -> the mask values the GPU produced on dom.FULL, for the last test of the sweep
_done = set()         # the geometries swept in this session


class _Device:
    """One device-mode call: every input uploaded, every output GUARD (+ its `shift`) bytes into a buffer of 0x5a of its own."""

    def __init__(self, torch, stream):
        self.torch, self.stream, self.ins, self.outs, self.ptr = torch, stream, {}, {}, {}

    def _place(self, nbytes, shift, content):
        t = self.torch.full((nbytes + 2 * GUARD + 16,), FILL, dtype=self.torch.uint8, device="cuda")
        off = GUARD + shift
        if content is not None:
            t[off:off + nbytes].copy_(self.torch.from_numpy(np.ascontiguousarray(content).view(np.uint8).reshape(-1).copy()))
        return t, off

    def input(self, name, a, shift=0):
        a = np.ascontiguousarray(a)
        t, off = self._place(a.nbytes, shift, a)
        self.ins[name] = (t, off, a)
        self.ptr[name] = t.data_ptr() + off
        return self.ptr[name]

    def output(self, name, dtype, shape, shift=0, init=None):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        t, off = self._place(nbytes, shift, init)
        self.outs[name] = (t, off, nbytes, np.dtype(dtype), tuple(shape), None if init is None else np.ascontiguousarray(init))
        self.ptr[name] = t.data_ptr() + off
        return self.ptr[name]

    def run(self, call):
        self.torch.cuda.synchronize()
        call(self.ptr, self.stream.cuda_stream)
        self.stream.synchronize()

    def results(self):
        """-> {name: array} after checking the guard bytes around every output and that every input still holds its bytes"""
        got = {}
        for name, (t, off, nbytes, dtype, shape, _) in self.outs.items():
            o = t.cpu().numpy()
            assert np.all(o[:off] == FILL) and np.all(o[off + nbytes:] == FILL), f"guard bytes around {name}"
            got[name] = o[off:off + nbytes].copy().view(dtype).reshape(shape)
        for name, (t, off, a) in self.ins.items():
            assert t.cpu().numpy()[off:off + a.nbytes].tobytes() == a.tobytes(), f"the input {name} was written to"
        return got

    def untouched(self):
        """nothing was written: every output buffer still holds its guard bytes and what it was given"""
        for name, (t, off, nbytes, _, _, init) in self.outs.items():
            o = t.cpu().numpy()
            body = o[off:off + nbytes]
            ok = np.all(o[:off] == FILL) and np.all(o[off + nbytes:] == FILL)
            ok = ok and (np.all(body == FILL) if init is None else body.tobytes() == init.tobytes())
            assert ok, f"a refused call wrote to {name}"


# ---- the stages: run(ctx, setting, mode) -> {name: array}; mode "host", "aligned", "odd" (device) or "inplace" (device) ----------
class _Ctx:
    def __init__(self, torch, eng, plain, c, w, h):
        self.torch, self.eng, self.plain, self.c, self.w, self.h = torch, eng, plain, c, w, h
        self.stream = torch.cuda.Stream()

    def dev(self):
        return _Device(self.torch, self.stream)


def _guide(ctx, d, odd, used):
    """(pointer, kind, pitch) of the luma guide of a device call: the int8 tensor with aligned buffers, the NV12 frames (pitch !=
    W) one byte off alignment otherwise; nothing when the setting reads no luma"""
    if not used:
        return 0, api.SN_GUIDE_NV12, 0
    if odd:
        return d.input("guide", ctx.c["nv"], 1), api.SN_GUIDE_NV12, ctx.c["pitch"]
    return d.input("guide", ctx.c["x"]), api.SN_GUIDE_TENSOR, 0


def _masked_outputs(d, shape, odd, per_map, disp0, raw=None):
    """out / mask / counter / disp of a masking stage; raw given: out starts as the input (the in-place call)"""
    d.output("out", np.int32, shape, 4 * odd, init=raw)
    d.output("mask", np.uint8, shape, odd)
    d.output("counts", np.uint32, (N,) + ((per_map,) if per_map > 1 else ()), 4 * odd)
    d.output("disp", np.float32, shape, 4 * odd, init=disp0)


def run_depth(ctx, s, mode):
    l, eng = ctx.c["l"], ctx.eng
    if mode == "host":
        r = eng.depth_from_raw(l, want_disp=s[0])
        return {"depth": r[0], "disp": r[1]} if s[0] else {"depth": r}
    d, odd = ctx.dev(), mode == "odd"
    d.input("raw", l)
    d.output("depth", np.float32, l.shape, 4 * odd)
    if s[0]:
        d.output("disp", np.float32, l.shape, 4 * odd)
    d.run(lambda p, st: eng._check(eng._lib.sn_depth_from_raw(eng._h, N, p["raw"], 527.1931762695312, 119.89382172, p["depth"],
                                                            p.get("disp"), api.SN_MEM_DEVICE, st), "sn_depth_from_raw"))
    return d


def run_pointcloud(ctx, s, mode):
    layout, step, colour = s
    l, eng, c = ctx.c["l"], ctx.eng, ctx.c
    cam = pointcloud.Camera(fx=dom.CAM.fx, fy=dom.CAM.fy, baseline_mm=dom.CAM.baseline_mm, step=step)
    if mode == "host":
        pts, counts = eng.pointcloud(l, cam, layout, c["nv"] if colour else None, c["pitch"] if colour else 0)
        return {"points": pts, "counts": counts}
    d, odd = ctx.dev(), mode == "odd"
    ho, wo = -(-ctx.h // max(step, 1)), -(-ctx.w // max(step, 1))
    d.input("raw", l)
    nv = d.input("nv", c["nv"], odd) if colour else 0
    d.output("points", np.float32, (N, ho, wo, 4) if layout == pointcloud.ORGANISED else (N, ho * wo, 4))      # 16-byte aligned by contract
    d.output("counts", np.uint32, (N,), 4 * odd)
    d.run(lambda p, st: eng.pointcloud_device(N, p["raw"], cam, p["points"], p["counts"], nv, c["pitch"] if colour else 0, layout, st))
    return d


def run_mirror(ctx, s, mode):
    x, eng = ctx.c["x"], ctx.eng
    if mode == "host":
        return {"out": eng.mirror_pair(x)}
    d = ctx.dev()
    d.input("in", x)
    d.output("out", np.int8, x.shape, mode == "odd")
    d.run(lambda p, st: eng.mirror_pair_device(N, p["in"], p["out"], st))
    return d


def run_lr_check(ctx, s, mode):
    tau_px, tau_rel, mirrored = s
    c, eng = ctx.c, ctx.eng
    l, r = c["l"], c["r_mirrored"] if mirrored else c["r"]
    if mode == "host":
        disp = c["disp0"].copy()
        out, mask, kept = eng.lr_check(l, r, tau_px, tau_rel, mirrored, disp)
        return {"out": out, "mask": mask, "kept": kept, "disp": disp}
    d, odd = ctx.dev(), mode == "odd"
    d.input("left", l)
    d.input("right", r)
    _masked_outputs(d, l.shape, odd, 1, c["disp0"])
    d.run(lambda p, st: eng.lr_check_device(N, p["left"], p["right"], tau_px, tau_rel, mirrored, p["out"], p["disp"], p["mask"], p["counts"], st))
    return d


def run_conf_mask(ctx, s, mode):
    c, eng = ctx.c, ctx.eng
    if mode == "host":
        disp = c["disp0"].copy()
        out, mask, kept = eng.conf_mask(c["l"], c["conf"], s[0], disp)
        return {"out": out, "mask": mask, "kept": kept, "disp": disp}
    d, odd = ctx.dev(), mode == "odd"
    d.input("raw", c["l"])
    d.input("conf", c["conf"])
    _masked_outputs(d, c["l"].shape, odd, 1, c["disp0"])
    d.run(lambda p, st: eng.conf_mask_device(N, p["raw"], p["conf"], s[0], p["out"], p["disp"], p["mask"], p["counts"], st))
    return d


def run_filter(ctx, s, mode):
    c, eng = ctx.c, ctx.eng
    l = c["l"]
    if mode == "host":
        disp = c["disp0"].copy()
        out, mask, counts = eng.filter_raw(l, *s, disp=disp)
        return {"out": out, "mask": mask, "counts": counts, "disp": disp}
    d, odd = ctx.dev(), mode == "odd"
    if mode != "inplace":
        d.input("raw", l)
    _masked_outputs(d, l.shape, odd, 3, c["disp0"], raw=l if mode == "inplace" else None)
    d.run(lambda p, st: eng.filter_raw_device(N, p.get("raw", p["out"]), *s, out_raw_ptr=p["out"], mask_ptr=p["mask"], disp_ptr=p["disp"],
                                              counts_ptr=p["counts"], stream=st))
    return d


def run_smooth(ctx, s, mode):
    radius, sigma, min_valid = s
    c, eng = ctx.c, ctx.eng
    l = c["l"]
    if mode == "host":
        disp = c["disp0"].copy()
        out, mask, counts = eng.smooth_raw(l, c["nv"] if sigma else None, api.SN_GUIDE_NV12, c["pitch"] if sigma else 0, radius, sigma,
                                           min_valid, disp=disp)
        return {"out": out, "mask": mask, "counts": counts, "disp": disp}
    d, odd = ctx.dev(), mode == "odd"
    if mode != "inplace":
        d.input("raw", l)
    guide, kind, pitch = _guide(ctx, d, odd, sigma > 0)
    _masked_outputs(d, l.shape, odd, 3, c["disp0"], raw=l if mode == "inplace" else None)
    d.run(lambda p, st: eng.smooth_raw_device(N, p.get("raw", p["out"]), guide, kind, pitch, radius, sigma, min_valid, out_raw_ptr=p["out"],
                                              mask_ptr=p["mask"], disp_ptr=p["disp"], counts_ptr=p["counts"], stream=st))
    return d


def run_temporal(ctx, s, mode):
    """two pushes of three maps on two streams: the second reads back the state the first left"""
    c, eng = ctx.c, ctx.eng
    got = {}
    with eng.temporal_filter(2, *s) as tf:
        for push, raw in enumerate((c["l"], c["r"])):
            ids = dom.temporal_ids(push)
            if mode == "host":
                disp = c["disp0"].copy()
                out, mask, counts = tf.push(raw, c["nv"] if s[3] else None, api.SN_GUIDE_NV12, c["pitch"] if s[3] else 0, ids, disp)
                one = {"out": out, "mask": mask, "counts": counts, "disp": disp}
            else:
                d, odd = ctx.dev(), mode == "odd"
                d.input("raw", raw)
                guide, kind, pitch = _guide(ctx, d, odd, s[3] > 0)
                _masked_outputs(d, raw.shape, odd, 4, c["disp0"])
                d.run(lambda p, st: tf.push_device(N, p["raw"], guide, kind, pitch, stream_of=ids, out_raw_ptr=p["out"], mask_ptr=p["mask"],
                                                   disp_ptr=p["disp"], counts_ptr=p["counts"], stream=st))
                one = d.results()
            got.update({f"{k}{push}": v for k, v in one.items()})
    return got


def run_render(ctx, s, mode):
    fmt, layout = s
    c, eng, w, h = ctx.c, ctx.eng, ctx.w, ctx.h
    prm = render.RenderParams(layout=layout)
    if mode == "host":
        return {"out": eng.render(c["l"], c["nv"], c["pitch"], prm, fmt)}
    d = ctx.dev()
    hc = h * (2 if layout == render.STACK else 1)
    rows, row_bytes = (hc + hc // 2, w) if fmt == render.NV12 else (hc, 3 * w)
    d.input("raw", c["l"])
    d.input("left", c["nv"])
    d.output("out", np.uint8, (N, rows, w) if fmt == render.NV12 else (N, hc, w, 3), mode == "odd")
    d.run(lambda p, st: eng.render_device(N, p["raw"], p["left"], c["pitch"], prm, fmt, p["out"], row_bytes, rows * row_bytes, st))
    return d


def run_rectifier(ctx, s, mode):
    c, eng, w, h = ctx.c, ctx.eng, ctx.w, ctx.h
    sw, sh = dom.SRC
    with eng.rectifier(c["calib"]) as rect:
        if mode == "host":
            sbs, ten = rect.rectify(c["src"], None, c["src_pitch"], N, want_tensor=True)
            return {"sbs": sbs, "tensor": ten}
        d, odd = ctx.dev(), mode == "odd"
        src = d.input("src", c["src"], odd)                       # the raw frames at an odd address
        d.output("sbs", np.uint8, (N, h + h // 2, 2 * w), 4 * odd)      # device outputs are 4-byte aligned by contract
        d.output("tensor", np.int8, (N, 6, h, w), 4 * odd)
        d.run(lambda p, st: rect.rectify_device(N, src, src + sw, c["src_pitch"], c["src_pitch"] * (sh + sh // 2), p["sbs"], p["tensor"], st))
        return d.results()


def run_obstacles(ctx, s, mode):
    eng = ctx.eng if s[0] == "rle" else ctx.plain
    l, p = ctx.c["l"], dom.OBSTACLE
    names = ("occ", "hits", "height", "ranges", "stats")
    if mode == "host":
        return dict(zip(names, eng.obstacles(l, dom.CAM, p)))
    d, odd = ctx.dev(), mode == "odd"
    d.input("raw", l)
    d.output("occ", np.int8, (N, p.gh, p.gw), odd)
    d.output("hits", np.uint32, (N, p.gh, p.gw, 2), 4 * odd)
    d.output("height", np.int32, (N, p.gh, p.gw), 4 * odd)
    d.output("ranges", np.float32, (N, p.beams), 4 * odd)
    d.output("stats", np.uint32, (N, 4), 4 * odd)
    d.run(lambda q, st: eng.obstacles_device(N, q["raw"], dom.CAM, p, q["occ"], q["hits"], q["height"], q["ranges"], q["stats"], st))
    return d


def run_ground(ctx, s, mode):
    from hobot_stereonet_amd import ground
    eng, l = ctx.eng, ctx.c["l"]
    if mode == "host":
        rec, lab = eng.ground(l, dom.CAM, dom.GROUND)
        return {"records": rec, "labels": lab}
    d = ctx.dev()
    d.input("raw", l)
    d.output("records", ground.RECORD, (N,))                       # 8-byte aligned by contract
    d.output("labels", np.uint8, l.shape, mode == "odd")
    d.run(lambda p, st: eng.ground_device(N, p["raw"], dom.CAM, dom.GROUND, p["records"], p["labels"], st))
    return d


RUN = {"depth": run_depth, "pointcloud": run_pointcloud, "mirror": run_mirror, "lr_check": run_lr_check, "conf_mask": run_conf_mask,
       "filter": run_filter, "smooth": run_smooth, "temporal": run_temporal, "render": run_render, "rectifier": run_rectifier,
       "obstacles": run_obstacles, "ground": run_ground}
RENAME = {"lr_check": {"counts": "kept"}, "conf_mask": {"counts": "kept"}}      # the device helper calls every counter `counts`
MODES = {"filter": ("host", "aligned", "odd", "inplace"), "smooth": ("host", "aligned", "odd", "inplace")}


def _outputs(stage, r):
    got = r.results() if isinstance(r, _Device) else r
    return {RENAME.get(stage, {}).get(k, k): v for k, v in got.items()}


def _refused(ctx, stage, s, mode):
    """the call of a refused (stage, setting, geometry): SN_ERR_ARG, nothing written"""
    if stage == "rectifier":
        calib = rectify.synthetic_rig(*dom.SRC, ctx.w, ctx.h, dom.SRC[0] + ctx.w)
        with pytest.raises(api.StereoNetError) as e:
            ctx.eng.rectifier(calib)
        assert e.value.code == -1, (stage, e.value)
        return
    if mode == "host":
        with pytest.raises(api.StereoNetError) as e:
            RUN[stage](ctx, s, mode)
        assert e.value.code == -1, (stage, s, e.value)
        return
    made = []
    real = ctx.dev

    def dev():
        made.append(real())
        return made[-1]

    ctx.dev = dev
    try:
        with pytest.raises(api.StereoNetError) as e:
            RUN[stage](ctx, s, mode)
    finally:
        ctx.dev = real
    assert e.value.code == -1 and len(made) == 1, (stage, s, e.value)
    ctx.stream.synchronize()
    made[0].untouched()


def _sweep(model_factory, w, h):
    """every stage, setting and mode at one geometry on one handle (and a second one created under SN_OBSTACLE_RLE=0, which
    sn_create reads: the plain accumulation of the obstacle grid) -> what differs from the twins"""
    import torch
    t0 = time.perf_counter()
    model = model_factory(w, h, dom.DMAX)
    before = os.environ.get("SN_OBSTACLE_RLE")
    os.environ["SN_OBSTACLE_RLE"] = "0"
    try:
        plain = api.StereoNetHIP(model, max_batch=N)
    finally:
        if before is None:
            del os.environ["SN_OBSTACLE_RLE"]
        else:
            os.environ["SN_OBSTACLE_RLE"] = before
    bad, report = [], []
    with plain, api.StereoNetHIP(model, max_batch=N) as eng:
        ctx = _Ctx(torch, eng, plain, dom.inputs(w, h), w, h)
        for stage, settings in dom.SETTINGS.items():
            compared = refused = differing = 0
            for s in settings:
                for mode in MODES.get(stage, ("host", "aligned", "odd")):
                    if (stage, s, (w, h)) in dom.REFUSALS:
                        _refused(ctx, stage, s, mode)
                        refused += 1
                        continue
                    want = dom.want(stage, s, w, h, eng.out_scale)
                    got = _outputs(stage, RUN[stage](ctx, s, mode))
                    diff = dom.differing(stage, s, got, want)
                    compared += 1
                    if diff:
                        differing += sum(diff.values())
                        bad.append((stage, s, mode, diff))
                    if (w, h) in dom.FULL and stage in dom.MASK_OF:
                        vals = set()
                        for k, v in got.items():
                            if k.startswith(dom.MASK_OF[stage]):
                                vals |= set(np.unique(v).tolist())
                        _seen.setdefault((stage, s), set()).update(vals)
            report.append(f"{stage} {compared} compared / {refused} refused / {differing} differing elements")
            if refused:      # the handle is still usable after whatever was refused: the plainest stage gives the twin's bits
                d0 = dom.differing("depth", (True,), run_depth(ctx, (True,), "host"), dom.want("depth", (True,), w, h, eng.out_scale))
                assert not d0, (stage, "the handle after a refusal", d0)
    _done.add((w, h))
    print(f"{w}x{h} ({dom.GEOMETRIES[(w, h)]}): " + "; ".join(report) + f"; {time.perf_counter() - t0:.2f} s")
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", GEOMS, ids=[f"{w}x{h}" for w, h in GEOMS])
def test_every_stage_equals_its_twin_at_this_geometry(model_factory, w, h):
    bad = _sweep(model_factory, w, h)
    assert not bad, bad


@pytest.mark.gpu
def test_the_gpu_masks_took_every_declared_value(model_factory):
    """Over the geometries of at least 63 x 15 the masks the GPU wrote hold exactly the declared values (the sweep above has
    recorded them; a geometry it has not run in this session is run here)."""
    for w, h in dom.FULL:
        if (w, h) not in _done:
            _sweep(model_factory, w, h)
    for key, declared in dom.MASK_VALUES.items():
        print(key, sorted(_seen.get(key, ())))
        assert _seen.get(key) == declared, (key, _seen.get(key))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", GEOMS, ids=[f"{w}x{h}" for w, h in GEOMS])
def test_infer_lrc_right_out_at_this_geometry(model_factory, w, h):
    """k_lr_check's right_out (the right eye's map in right-image coordinates) is reached through sn_infer_lrc alone: the
    composite equals the twin's check of the two maps sn_infer_batch gives for the pair and the mirrored pair, in host mode and in
    device mode with right_out, mask and kept aligned and one element or byte off (the maps the forward pass writes stay aligned)."""
    import torch
    from hobot_stereonet_amd import lrcheck, synth
    x = np.stack([synth.model_input_i8(w, h, dom.DMAX, 7 + k) for k in range(N)])
    taus = (0.5, 0.02)
    with api.StereoNetHIP(model_factory(w, h, dom.DMAX), max_batch=N, precision=api.PREC_FP32) as eng:
        d_l, r_l = eng.infer(x)
        _, r_m = eng.infer(eng.mirror_pair(x))
        raw, mask, kept = lrcheck.reference(r_l, r_m, *taus, True, eng.out_scale)
        want = {"raw": raw, "mask": mask, "kept": kept, "right": np.ascontiguousarray(r_m[..., ::-1]),
                "disp": np.where(mask != 0, np.uint32(0), d_l.view(np.uint32)).view(np.float32)}
        disp, raw, mask, kept, right = eng.infer_lrc(x, *taus, want_right=True)
        diffs = {"host": dom.differing("infer_lrc", (), {"raw": raw, "mask": mask, "kept": kept, "right": right, "disp": disp}, want)}
        stream = torch.cuda.Stream()
        for mode in ("aligned", "odd"):
            d, odd = _Device(torch, stream), mode == "odd"
            d.input("in", x)
            d.output("raw", np.int32, r_l.shape)
            d.output("disp", np.float32, r_l.shape)
            d.output("right", np.int32, r_l.shape, 4 * odd)
            d.output("mask", np.uint8, r_l.shape, odd)
            d.output("kept", np.uint32, (N,), 4 * odd)
            d.run(lambda p, st: eng.infer_lrc_device(N, p["in"], *taus, p["raw"], p["disp"], p["right"], p["mask"], p["kept"], stream=st))
            diffs[mode] = dom.differing("infer_lrc", (), d.results(), want)
    print(f"{w}x{h}: kept {want['kept'].tolist()} of {w * h}, mask values {np.unique(want['mask']).tolist()}, differing elements {diffs}")
    assert not any(diffs.values()), diffs


# ---- the slice walks: more maps in one push than a launch takes --------------------------------------------------------------------
SLICE = 64                 # kSlice (csrc/sn_stream_groups.hpp)
BIG, SECOND = 130, 70


def _walk_ids():
    """130 maps on three streams: 0 and 1 alternate in the first launch, all three take turns in the second (stream 2 appears
    there first, `fresh` for it alone), the third launch (2 maps) holds streams 2 and 0; then 70 maps of all three in turn"""
    first = [k % 2 for k in range(SLICE)] + [k % 3 for k in range(SLICE, 2 * SLICE)] + [2, 0]
    assert len(first) == BIG and 2 not in first[:SLICE] and {0, 1, 2} == set(first[SLICE:2 * SLICE])
    return first, [k % 3 for k in range(SECOND)]


def _launches(n):
    return [min(SLICE, n - k0) for k0 in range(0, n, SLICE)]


@pytest.mark.gpu
@pytest.mark.parametrize("luma_delta", [24, 0], ids=["guide-nv12-pitch10", "no-guide"])
def test_temporal_push_walks_three_slices(model_factory, luma_delta):
    w = h = 8
    setting = (64, 1.0, 2, luma_delta)
    rng = np.random.default_rng(130 + luma_delta)
    S = float(temporal.wire_scale())
    surf = rng.uniform(2.0, 6.0, (h, w))
    raw = np.rint((surf[None] + rng.normal(0, 0.4, (BIG, h, w))) / S).astype(np.int32)
    raw[rng.random(raw.shape) < 0.2] = 0
    raw[rng.random(raw.shape) < 0.03] = -7
    pitch = w + 2
    nv = rng.integers(0, 256, (BIG, h + (h + 1) // 2, pitch), dtype=np.uint8)
    nv[:, :h, :w] = np.clip(100 + rng.integers(-20, 21, (BIG, h, w)), 0, 255)      # consecutive frames differ by up to 40: some move
    luma = smooth.luma_from_nv12(nv, w, h, pitch, BIG)
    ids1, ids2 = _walk_ids()
    disp0 = rng.integers(0, 2 ** 32, raw.shape, dtype=np.uint32).view(np.float32)
    states = {}
    want1 = temporal.reference(raw, luma if luma_delta else None, setting, ids1, states)
    del states[1]                                                  # reset(1)
    want2 = temporal.reference(raw[:SECOND], luma[:SECOND] if luma_delta else None, setting, ids2, states)
    print(f"launches of the two pushes: {_launches(BIG)} and {_launches(SECOND)} maps; mask values {np.unique(want1[1]).tolist()}")
    assert _launches(BIG) == [64, 64, 2] and _launches(SECOND) == [64, 6]
    assert set(np.unique(want1[1]).tolist()) == ({0, 1, 2, 5, 8, 9, 16} if luma_delta else {0, 1, 2, 5, 16})
    with api.StereoNetHIP(model_factory(w, h, dom.DMAX), max_batch=BIG) as eng, eng.temporal_filter(3, *setting) as tf:
        guide = (nv, api.SN_GUIDE_NV12, pitch) if luma_delta else (None, api.SN_GUIDE_NV12, 0)
        disp = disp0.copy()
        got1 = tf.push(raw, *guide, ids1, disp)
        tf.reset(1)
        got2 = tf.push(raw[:SECOND], None if guide[0] is None else guide[0][:SECOND], guide[1], guide[2], ids2)
    for tag, got, want in (("130 maps", got1, want1), ("70 maps after reset(1)", got2, want2)):
        diff = [int((g != t).sum()) for g, t in zip(got, want)]
        print(f"{tag}: differing elements (out, mask, counts) = {diff}; per launch {[int((got[1][k0:k0 + SLICE] != want[1][k0:k0 + SLICE]).sum()) for k0 in range(0, len(got[1]), SLICE)]}")
        assert diff == [0, 0, 0], tag
    assert np.array_equal(disp.view(np.uint32), temporal.expected_disp(disp0, raw, want1[0]).view(np.uint32))


@pytest.mark.gpu
def test_costmap_push_walks_three_slices(model_factory):
    op = obstacles.ObstacleParams(x_min_m=-0.5, y_min_m=-1.0, cell_m=0.25, gw=5, gh=8, beams=8, angle_min_rad=-0.8, angle_increment_rad=0.2)
    p = costmap.CostmapParams(mw=24, mh=18, l_hit=90, l_miss=55, l_min=-130, l_max=170, clear_margin_m=0.2, clear_min_m=0.3, clear_max_m=0.0)
    poses, occ, ranges = costmap.synthetic_clip(p, op, BIG, seed=13)      # a random walk: the window scrolls by a cell or two per frame
    ids1, ids2 = _walk_ids()
    twin = costmap.Reference(p, op, 3, edges=api.beam_edges(op))
    with api.StereoNetHIP(model_factory(8, 8, dom.DMAX), max_batch=BIG) as eng, eng.costmap(op, p, streams=3) as cm:
        got1 = cm.push(poses, occ, ranges, ids1)
        want1 = twin.push(got1[3], occ, ranges, ids1)
        cm.reset(1)
        twin.reset(1)
        got2 = cm.push(poses[:SECOND][::-1], occ[:SECOND], ranges[:SECOND], ids2)      # the walk backwards: other origins than before
        want2 = twin.push(got2[3], occ[:SECOND], ranges[:SECOND], ids2)
    # the window moved inside every launch and across each boundary between two launches, on the stream that crosses it
    frames = twin.frames[:BIG]
    moved = [f["prev"] not in (None, f["origin"]) for f in frames]
    assert all(any(moved[k0:k0 + m]) for k0, m in zip(range(0, BIG, SLICE), _launches(BIG))), moved
    for k0 in (SLICE, 2 * SLICE):
        k = next(k for k in range(k0, BIG) if ids1[k] in ids1[:k0])       # the first map of the launch whose stream has a past
        assert frames[k]["prev"] is not None
    tot = {k: sum(f[k] for f in twin.frames) for k in ("hit", "clear_occ", "clear_ray", "scrolled")}
    print(f"launches {_launches(BIG)} and {_launches(SECOND)} maps; branches taken {tot}")
    assert all(v > 0 for v in tot.values()), tot
    for tag, got, want in (("130 maps", got1, want1), ("70 maps after reset(1)", got2, want2)):
        diff = [int((g != t).sum()) for g, t in zip(got[:3], want)]
        print(f"{tag}: differing elements (grid, logodds, stats) = {diff}")
        assert diff == [0, 0, 0], tag
