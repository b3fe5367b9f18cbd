"""The premises of tests/test_gpu_postproc_geometry.py, checked without a GPU on the geometries of
tests/golden/postproc_domain.py: every numpy twin agrees there with the independent plain-loop or scalar reference the project has
for it (tests/golden/plain_refs.py, ground.reference_loops, the host C++ canvas and the library's rectification map), the inputs
make every mask take every value its setting can produce and every counter count, and the table of refused calls is the one the
header's contract gives.  The degenerate geometries are compared like the others; only the non-vacuity is asked of the larger ones."""
import dataclasses

import numpy as np
import pytest

import plain_refs
import postproc_domain as dom
from hobot_stereonet_amd import api, dispfilter, ground, obstacles, rectify, render, temporal

GEOMS = list(dom.GEOMETRIES)
IDS = [f"{w}x{h}" for w, h in GEOMS]


def test_the_geometry_list_and_the_inputs():
    assert set(dom.DEGENERATE) <= set(GEOMS) and len(dom.FULL) == 7 and not set(dom.FULL) & set(dom.DEGENERATE)
    assert all(len(why) > 20 for why in dom.GEOMETRIES.values())      # every geometry says which constant it is there for
    for w, h in GEOMS:
        c = dom.inputs(w, h)
        l, r = c["l"], c["r"]
        assert l.shape == r.shape == (dom.N, h, w) and l.dtype == np.int32
        assert c["pitch"] != w and c["pitch"] % 2 == 0 and np.isnan(c["conf"]).sum() == 1
        assert np.array_equal(c["x"][:, 0].view(np.uint8) ^ np.uint8(0x80), c["luma"])       # both guide forms carry one luma
        if h * w >= 8:
            assert l[0].reshape(-1)[:4].tolist() == [dom.IMIN, 0, 1, dom.IMAX] and l[-1].reshape(-1)[-4:].tolist() == [dom.IMAX, 1, 0, dom.IMIN]
        if (w, h) in dom.FULL:
            frac = float((l <= 0).mean())
            print(f"{w}x{h}: {frac:.3f} of the pixels <= 0, {int((l < 0).sum())} negative")
            assert 0.2 < frac < 0.3 and (l < 0).sum() > 3


def _same(tag, got, want):
    for k, (g, t) in enumerate(zip(got, want)):
        g, t = np.asarray(g), np.asarray(t)
        assert g.shape == t.shape, (tag, k)
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, t.view(np.uint32) if t.dtype == np.float32 else t), (tag, k)


def _each(stage, w, h):
    return [(i, s) for i, s in enumerate(dom.SETTINGS[stage]) if dom.refusal(stage, s, w, h) is None]


@pytest.mark.parametrize("w,h", GEOMS, ids=IDS)
def test_filter_twin_equals_flood_fill_and_scalar_fill(w, h):
    l = dom.inputs(w, h)["l"]
    for _, s in _each("filter", w, h):
        t = dom.want("filter", s, w, h)
        for k in range(dom.N):
            out, mask = plain_refs.filter_independent(l[k], s[0], dispfilter.diff_units(s[1]), s[2])
            _same(("filter", s, k), (t["out"][k], t["mask"][k]), (out, mask))


@pytest.mark.parametrize("w,h", GEOMS, ids=IDS)
def test_smooth_twin_equals_the_per_pixel_loop(w, h):
    c = dom.inputs(w, h)
    for i, s in _each("smooth", w, h):
        t = dom.want("smooth", s, w, h)
        k = i % dom.N               # the loop takes a second per map at the largest geometry: every setting on one map, every map used
        _same(("smooth", s, k), (t["out"][k], t["mask"][k]), plain_refs.smooth_brute(c["l"][k], c["luma"][k], *s))


@pytest.mark.parametrize("w,h", GEOMS, ids=IDS)
def test_temporal_twin_equals_the_per_pixel_loop(w, h):
    c = dom.inputs(w, h)
    frames = [(p, k) for p in (0, 1) for k in range(dom.N)]             # (push, map) in the order the filter sees them
    for _, s in _each("temporal", w, h):
        t = dom.want("temporal", s, w, h)
        for stream in (0, 1):
            mine = [(p, k) for p, k in frames if dom.temporal_ids(p)[k] == stream]
            assert len(mine) == 3
            raw = np.stack([(c["l"], c["r"])[p][k] for p, k in mine])
            luma = np.stack([c["luma"][k] for _, k in mine])
            out, mask = plain_refs.temporal_loop(raw, luma, s[0], dispfilter.diff_units(s[1]), s[2], s[3])
            _same(("temporal", s, stream), (np.stack([t[f"out{p}"][k] for p, k in mine]), np.stack([t[f"mask{p}"][k] for p, k in mine])),
                  (out, mask))
            assert np.array_equal(np.stack([t[f"counts{p}"][k] for p, k in mine]), temporal.counts_of(out, mask))


@pytest.mark.parametrize("w,h", GEOMS, ids=IDS)
def test_lr_check_twin_equals_the_scalar_contract(w, h):
    c = dom.inputs(w, h)
    for _, s in _each("lr_check", w, h):
        t = dom.want("lr_check", s, w, h)
        for k in range(dom.N):
            out, mask, kept = plain_refs.lrcheck_scalar(c["l"][k], (c["r_mirrored"] if s[2] else c["r"])[k], *s)
            _same(("lr_check", s, k), (t["out"][k], t["mask"][k], t["kept"][k]), (out, mask, kept))


@pytest.mark.parametrize("w,h", GEOMS, ids=IDS)
def test_obstacle_twin_equals_the_scalar_loop(w, h):
    t = dom.want("obstacles", ("rle",), w, h)
    got = plain_refs.obstacles_scalar_loop(dom.inputs(w, h)["l"], dom.CAM.resolved(w, h), dom.OBSTACLE, api.beam_edges(dom.OBSTACLE))
    _same("obstacles", [t[k] for k in ("occ", "hits", "height", "ranges", "stats")], got)
    assert all(np.array_equal(a, b) for a, b in zip(dom.want("obstacles", ("plain",), w, h).values(), t.values()))


@pytest.mark.parametrize("w,h", GEOMS, ids=IDS)
def test_ground_twin_equals_the_plain_loops(w, h):
    if dom.refusal("ground", (), w, h):
        with pytest.raises(ValueError):
            ground.roi(dom.GROUND, w, h, 1)
        return
    t = dom.want("ground", (), w, h)
    rec, lab = ground.reference_loops(dom.inputs(w, h)["l"], dom.CAM, dom.GROUND, gate_q16=api.ground_gate(dom.CAM, dom.GROUND, w, h))
    assert rec.tobytes() == t["records"].tobytes(), (rec, t["records"])
    assert np.array_equal(lab, t["labels"])


@pytest.mark.parametrize("w,h", GEOMS, ids=IDS)
def test_render_twin_equals_host_cpp(w, h):
    c = dom.inputs(w, h)
    left = np.ascontiguousarray(c["nv"]).reshape(-1)
    for i, (fmt, layout) in _each("render", w, h):
        got = plain_refs.host_canvas(dom.N, c["l"], left, c["pitch"], w, h, render.RenderParams(layout=layout), fmt, pad=(0, 6)[i & 1])
        want = dom.want("render", (fmt, layout), w, h)["out"]
        assert got.shape == want.shape and np.array_equal(got, want), (fmt, layout)


@pytest.mark.parametrize("w,h", GEOMS, ids=IDS)
def test_rectification_map_of_the_library_equals_the_twin(w, h):
    if dom.refusal("rectifier", (), w, h):
        assert "calib" not in dom.inputs(w, h)
        return
    calib = dom.inputs(w, h)["calib"]
    for eye in (0, 1):
        want = rectify.build_map(calib, eye, w, h)
        got = api.rectify_build_map(calib, eye, w, h)
        print(f"{w}x{h} eye {eye}: {rectify.nonvacuity(want, *dom.SRC)}")
        assert got.dtype == np.int32 and got.shape == (h, w, 2) and np.array_equal(got, want)
    t = dom.want("rectifier", (), w, h)
    assert t["sbs"].shape == (dom.N, h + h // 2, 2 * w) and t["tensor"].shape == (dom.N, 6, h, w)


def test_every_mask_value_and_every_counter_occurs_on_the_larger_geometries():
    """Non-vacuity: over the geometries of at least 63 x 15 each setting's mask takes exactly the declared values and every
    counter is non-zero somewhere, so that the GPU comparison cannot pass on an idle stage."""
    per_stage = {}
    for (stage, s), declared in dom.MASK_VALUES.items():
        seen, counters = set(), None
        for w, h in dom.FULL:
            t = dom.want(stage, s, w, h)
            names = [k for k in t if k.startswith(dom.MASK_OF[stage])]
            seen |= set(np.unique(np.concatenate([t[k].reshape(-1) for k in names])).tolist())
            if stage in dom.COUNTERS_OF:
                cn = np.concatenate([t[k].reshape(dom.N, -1) for k in t if k.startswith(dom.COUNTERS_OF[stage])]).astype(np.int64).sum(0)
                counters = cn if counters is None else counters + cn
        print(f"{stage} {s}: mask values {sorted(seen)}, counters {None if counters is None else counters.tolist()}")
        assert seen == declared, (stage, s, sorted(seen))
        if counters is not None:      # a counter of a stage that the setting switches off stays 0: it must count under another setting
            per_stage[stage] = per_stage.get(stage, 0) + counters
    assert set(per_stage) == set(dom.COUNTERS_OF) - {"pointcloud"} and all(np.all(c > 0) for c in per_stage.values()), per_stage
    for w, h in dom.FULL:
        for s in dom.SETTINGS["pointcloud"]:
            if dom.refusal("pointcloud", s, w, h) is None:
                cnt, (ho, wo) = dom.want("pointcloud", s, w, h)["counts"], dataclasses.replace(dom.CAM, step=s[1]).out_shape(w, h)
                assert np.all(cnt > 0) and np.all(cnt < ho * wo), (w, h, s)
        rec = dom.want("ground", (), w, h)["records"]
        ob = dom.want("obstacles", ("rle",), w, h)
        print(f"{w}x{h}: ground flags {rec['flags'].tolist()} inliers {rec['inliers'].tolist()}, obstacle stats {ob['stats'].sum(0).tolist()}, "
              f"beams with a return {int(np.isfinite(ob['ranges']).sum())}")
        assert (rec["flags"] & ground.FOUND).any() and np.isfinite(ob["ranges"]).any() and np.isinf(ob["ranges"]).any()
        assert (ob["height"] > obstacles.NO_HEIGHT).any()
        depth = dom.want("depth", (True,), w, h)["depth"]
        assert np.isinf(depth).any() and np.isfinite(depth).any() and (depth < 0).any()
    # the compact tile's three geometries hold one sample less, exactly and one more than a tile at step 1
    assert [w * h for w, h in ((65, 63), (64, 64), (241, 17))] == [4095, 4096, 4097]


def test_the_refusal_table_is_the_headers():
    """Every (stage, setting, geometry) is either compared or refused; the refused ones are those the header's contract names, and
    where a twin checks the same sentence it raises for exactly them."""
    known = {("filter", (6, 1.0, 0), (1, 1)), ("filter", (6, 1.0, 0), (2, 2)), ("filter", (40, 0.5, 16), (5, 3)),
             ("render", (render.NV12, render.STACK), (65, 17)), ("render", (render.NV12, render.DEPTH), (70, 1)),
             ("rectifier", (), (2, 2)), ("rectifier", (), (63, 15)), ("rectifier", (), (70, 1)), ("ground", (), (1, 1)), ("ground", (), (2, 2)),
             ("pointcloud", (0, 3, 0), (64, 64))}
    assert known <= set(dom.REFUSALS)
    assert ("filter", (40, 0.5, 16), (1, 40)) not in dom.REFUSALS and ("ground", (), (5, 3)) not in dom.REFUSALS      # 40 = H*W; 10 samples
    assert ("rectifier", (), (256, 2)) not in dom.REFUSALS and ("render", (render.NV12, render.STACK), (2, 2)) not in dom.REFUSALS
    header = open(plain_refs.ROOT + "/include/stereonet_hip.h").read()
    for words in ("speckle_max_px outside 0..H*W", "W and H must be even", "W % 4 != 0 or an odd H is SN_ERR_ARG",
                  "holds fewer than three samples", "step not 1/2/4"):
        assert words in header, words
    compared = refused = 0
    for stage, settings in dom.SETTINGS.items():
        for s in settings:
            for w, h in GEOMS:
                if (stage, s, (w, h)) in dom.REFUSALS:
                    refused += 1
                    c = dom.inputs(w, h)
                    if stage in ("filter", "render", "ground"):
                        with pytest.raises(ValueError):
                            {"filter": lambda: dispfilter.reference(c["l"], *s),
                             "render": lambda: render.canvas(c["l"], c["nv"], c["pitch"], render.RenderParams(layout=s[1]), s[0]),
                             "ground": lambda: ground.reference(c["l"], dom.CAM, dom.GROUND, gate_q16=np.zeros(6, np.int64))}[stage]()
                else:
                    compared += 1
                    assert dom.want(stage, s, w, h)
    print(f"{compared} (stage, setting, geometry) triples compared, {refused} refused")
    assert compared + refused == sum(len(v) for v in dom.SETTINGS.values()) * len(GEOMS) and refused == len(dom.REFUSALS)
