"""Every persistent kernel of the towers and the low-resolution convolutions at small grids and batches: the sn_dbg_* hooks
launch each kernel as the pipeline does, sn_dbg_set_grid_cus caps the CU count their launchers see, so that a tensor of at most
64 x 320 runs the tile loops, the tile queue, the XCD bands and the share boundaries of the streamed blocks that otherwise only
the 720 x 1280 cases reach.  References and cases: tests/golden/tower_ref.py; tests/test_tower_refs.py proves on the CPU that the
inputs called exact are exact in any summation order, that the outputs have no equal rows, and that the criteria used here reject
an unwritten row, a restarted unit, swapped strips / row phases / images, a skipped tile and a misplaced channel block.

Judgement.  Exact family: bit-equal to the float64 reference at every cap.  Random family: at the default grid the bound the
kernel's existing test uses (quoted at each case); at every other cap bit-equal to the default grid's result and to the
two-launch form where there is one (the maps are the same bits for any workgroup count).  Every hook call also checks
the zero borders, front rows and slack of its tensors (SN_ERR_DEVICE otherwise) and starts its output as NaN.

n: the streamed blocks run n = 1 and 3.  The banded kernels run the n of {1, 2} at which cap 8 still gives every workgroup three
tiles on a tensor of at most 64 x 320 with two or three tiles in x: two workgroups per CU on 8 x 64 tiles need n = 2.
Needs an MI355X.  The lines starting with `tower_grid` are the record in profiles/tower_grid_parity.txt."""
import numpy as np
import pytest
import torch

import tower_ref as tr
from hobot_stereonet_amd import api

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


def _engine(model_factory, prec):
    eng = api.StereoNetHIP(model_factory(96, 64, 48), max_batch=2, precision=prec)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def eng16(model_factory):
    yield from _engine(model_factory, api.PREC_F16)


@pytest.fixture(scope="module")
def engx3(model_factory):
    yield from _engine(model_factory, api.PREC_F16X3)


@pytest.fixture(scope="module")
def eng32(model_factory):
    yield from _engine(model_factory, api.PREC_FP32)


@pytest.fixture(scope="module")
def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _at(eng, cus, fn):
    """fn() with the hooks' grid capped at `cus` CUs (0 = the device's) -> (result, workgroups, units)"""
    eng.dbg_set_grid_cus(cus)
    try:
        out = fn()
    finally:
        eng.dbg_set_grid_cus(0)
    return (out,) + eng.dbg_last_launch()


def _finite(out):
    return all(np.isfinite(np.asarray(o, F64)).all() for o in (out if isinstance(out, tuple) else (out,)))


def _same(a, b):
    if isinstance(a, tuple):
        return all(tr.same_bits(x, y) for x, y in zip(a, b))
    return tr.same_bits(a, b)


def test_the_cap_is_checked_and_banded_hooks_want_whole_bands(eng16, num_cu):
    with pytest.raises(api.StereoNetError):
        eng16.dbg_set_grid_cus(num_cu + 1)
    with pytest.raises(api.StereoNetError):
        eng16.dbg_set_grid_cus(-1)
    x, w, b, _ = tr.exact_f16_layer(1, 16, 70, 0)
    ref = tr.layer_f16(x, w, b, 1).astype(F32)
    for cus in (12, 1):          # no multiple of 8: k_ref_conv_f16_v2's launcher builds XCD bands
        with pytest.raises(api.StereoNetError, match="multiple of 8"):
            _at(eng16, cus, lambda: eng16.dbg_ref_conv_f16(x, w, b, 1, lrelu=True))
    got, wgs, units = _at(eng16, 8, lambda: eng16.dbg_ref_conv_f16(x, w, b, 1, lrelu=True, tile_w=64))
    assert (wgs, units) == (8, 4) and tr.same_bits(got, ref)          # 2 x 2 tiles in one image: one band of 8, four tiles
    x5, w1, b1, w2, b2 = tr.exact_f16_block(1, 7, 70, 0)
    got, wgs, units = _at(eng16, 5, lambda: eng16.dbg_ref_block_f16(x5, w1, b1, w2, b2, 1, fused=2))      # streamed: any cap
    assert (wgs, units) == (5, 14) and tr.same_bits(got, tr.block_f16(x5, w1, b1, w2, b2, 1).astype(F32))


# ---- streamed blocks: every distinct rows_per_wg from one row per workgroup to the whole launch in one ----------------
def _stream_sweep(eng, num_cu, n, h, w, dil, ow, tag, exact_fn, exact_ref, rand_fn, rand_ok, two_launch):
    """exact_fn / rand_fn: () -> hook result at the current cap; rand_ok(result) -> (passed, figure) at the default grid.
    The caps are the smallest one for every distinct rows_per_wg, from 1 (the whole launch in one workgroup) to total_rows (one
    row each) — or to the device's CU count where the launch has more rows than that (n = 3 at dilation 8: two rows each)."""
    total = tr.stream_sched(n, h, w, dil, ow, num_cu)["total"]
    caps = tr.stream_caps(total, num_cu)
    base, wgs0, units0 = _at(eng, 0, rand_fn)
    ok, figure = rand_ok(base)
    assert units0 == total
    assert _finite(base) and ok, (tag, figure)
    assert _same(base, two_launch()), tag          # the two-launch form at the default grid
    events, smallest = set(), None
    for cap in caps:
        s = tr.stream_sched(n, h, w, dil, ow, cap)
        got, wgs, units = _at(eng, cap, exact_fn)
        assert (wgs, units) == (s["grid"], total), (tag, cap, wgs, units, s)      # the launch is the schedule the events are read from
        assert _finite(got) and _same(got, exact_ref), (tag, cap, "exact")
        got, _, _ = _at(eng, cap, rand_fn)
        assert _finite(got) and _same(got, base), (tag, cap, "random")
        events |= tr.stream_events(s)
        smallest = smallest or (cap, units, wgs)
    want = tr.STREAM_EVENTS - (set() if n > 1 else {"image_boundary"})
    assert want <= events, (tag, want - events)
    print(f"tower_grid {tag} n={n} {h}x{w}: caps {caps[0]}..{caps[-1]} ({len(caps)} values of rows_per_wg), at cap {smallest[0]} "
          f"{smallest[1]} flat rows on {smallest[2]} workgroup(s), default grid {wgs0} workgroups; random family at the default "
          f"grid: {figure}")


@pytest.mark.parametrize("n", tr.STREAM_N)
@pytest.mark.parametrize("dil,h,w", tr.STREAM_F16)
def test_streamed_f16_block_at_every_share_size(eng16, num_cu, dil, h, w, n):
    """k_ref_block_stream_f16.  Random family at the default grid: max <= 3e-3 scale and mean < 3e-4 scale against the block with t
    rounded to fp16 (tests/test_gpu_f16.py::test_residual_block_f16)."""
    ex = tr.exact_f16_block(n, h, w, 100 + dil)
    rd = tr.random_block(n, h, w, 200 + dil, fp16=True)
    truth = tr.truth_block(*rd, dil, round_t=tr.q16)

    def ok(got):
        err, scale = np.abs(got - truth), np.abs(truth).max()
        return err.max() <= 3e-3 * scale and err.mean() < 3e-4 * scale, f"max {err.max() / scale:.2e} mean {err.mean() / scale:.2e} of scale"

    _stream_sweep(eng16, num_cu, n, h, w, dil, tr.STREAM_OW_F16[dil], f"k_ref_block_stream_f16 dil {dil}",
                  lambda: eng16.dbg_ref_block_f16(*ex, dil, fused=2), tr.block_f16(*ex, dil).astype(F32),
                  lambda: eng16.dbg_ref_block_f16(*rd, dil, fused=2), ok, lambda: eng16.dbg_ref_block_f16(*rd, dil, fused=0))


@pytest.mark.parametrize("n", tr.STREAM_N)
@pytest.mark.parametrize("dil,h,w", tr.STREAM_X3)
def test_streamed_split_block_at_every_share_size(engx3, num_cu, dil, h, w, n):
    """k_ref_block_stream_x3.  Random family at the default grid: max <= 2e-5 max|ref| (tests/test_gpu_x3_stream.py)."""
    ex = tr.exact_x3_block(n, h, w, 300 + dil)
    rd = tr.random_block(n, h, w, 400 + dil)
    truth = tr.truth_block(*rd, dil)
    _stream_sweep(engx3, num_cu, n, h, w, dil, tr.STREAM_OW_X3[dil], f"k_ref_block_stream_x3 dil {dil}",
                  lambda: engx3.dbg_ref_block_f16x3(*ex, dil, streamed=True), tr.block_x3(*ex, dil),
                  lambda: engx3.dbg_ref_block_f16x3(*rd, dil, streamed=True),
                  lambda got: (tr.within(got, truth, 2e-5), f"max {tr.max_rel(got, truth):.2e} of max|ref|"),
                  lambda: engx3.dbg_ref_block_f16x3(*rd, dil, streamed=False))


@pytest.mark.parametrize("n", tr.STREAM_N)
def test_tail_form_at_every_share_size(eng16, num_cu, n):
    """The tail form (last block + head in one launch, 60-column strips).  Random family at the default grid: mean < 2e-4 px and
    max < 5e-3 px against the block + head arithmetic (tests/test_gpu_tail.py::test_tail_form_vs_oracle_arithmetic)."""
    from test_gpu_tail import _operands
    hk, wk, ho, wo, ups = tr.STREAM_TAIL
    ex = tr.exact_f16_tail(n, hk, wk, ups, 500)
    eref = tr.tail_f16(*ex, ups, 64.0, ho, wo)
    rd = _operands(501, n, hk, wk, ups)
    truth = tr.tail_f16(*rd, ups, 192.0, ho, wo)["disp"]

    def ok(got):
        err = np.abs(got[0] - truth)
        return err.mean() < 2e-4 and err.max() < 5e-3 and bool((got[1] >= 0).all()), f"mean {err.mean():.2e} max {err.max():.2e} px"

    _stream_sweep(eng16, num_cu, n, ho, wo, 1, tr.STREAM_OW_TAIL, "k_ref_block_stream_f16 tail form",
                  lambda: eng16.dbg_ref_tail_f16(*ex, ups, 64.0, ho, wo, form=1), (eref["disp"].astype(F32), eref["raw"]),
                  lambda: eng16.dbg_ref_tail_f16(*rd, ups, 192.0, ho, wo, form=1), ok,
                  lambda: eng16.dbg_ref_tail_f16(*rd, ups, 192.0, ho, wo, form=0))


# ---- banded kernels: caps 8, 16, 24, 64 ----------------------------------------------------------------------------------
def _banded_sweep(eng, tag, exact_fn, exact_ref, rand_fn, rand_ok, twin=None):
    """twin: () -> the result of another kernel that must give the same bits (the plain-layout kernel for the zero-bordered one)"""
    base, wgs0, units0 = _at(eng, 0, rand_fn)
    ok, figure = rand_ok(base)
    assert _finite(base) and ok, (tag, figure)
    got, _, _ = _at(eng, 0, exact_fn)
    assert _finite(got) and _same(got, exact_ref), (tag, "default grid", "exact")
    at8 = None
    for cap in tr.CAPS:
        got, wgs, units = _at(eng, cap, exact_fn)
        assert _finite(got) and _same(got, exact_ref), (tag, cap, "exact")
        at8 = at8 or (units, wgs)
        assert units == units0 and wgs <= max(wgs0, 8), (tag, cap, wgs, units)
        got, _, _ = _at(eng, cap, rand_fn)
        assert _finite(got) and _same(got, base), (tag, cap, "random")
    assert at8[0] >= 3 * at8[1], (tag, "cap 8 must give every workgroup three units", at8)
    if twin is not None:
        assert _same(base, twin()), (tag, "twin kernel")
    print(f"tower_grid {tag}: caps {tr.CAPS}, at cap 8 {at8[0]} units on {at8[1]} workgroups, default grid {wgs0} workgroups; random "
          f"family at the default grid: {figure}")


def _rel(truth, bound):
    return lambda got: (tr.within(got, truth, bound), f"max {tr.max_rel(got, truth):.2e} of max|ref| (bound {bound:.0e})")


# (dil, tile width forced, h, w): three tiles in x, the last one a few columns wide; 8 tile rows, the last one 4 rows high
F16_LAYER = [(1, 64, 60, 130), (1, 32, 60, 70), (2, 64, 60, 130), (2, 32, 60, 70), (4, 0, 60, 70), (8, 0, 60, 70)]


@pytest.mark.parametrize("res", [False, True], ids=["conv1", "conv2_residual"])
@pytest.mark.parametrize("dil,tw,h,w", F16_LAYER)
def test_f16_layer_tile_queue_at_small_grids(eng16, dil, tw, h, w, res):
    """k_ref_conv_f16_v2, both tile widths, n = 2: 48 tiles, so at cap 8 (16 workgroups) everyone takes a third tile from the queue.
    Random family at the default grid (tests/test_gpu_f16.py::test_ref_conv_f16_layer): without residual and activation
    |got - fp16(ref)| <= 1e-3 scale + 1e-6 and mean |got - ref| < 3e-4 scale; residual + LeakyReLU: max <= 1.2e-3 max|ref| + 1e-6."""
    n = 2
    x, wt, b, r = tr.exact_f16_layer(n, h, w, 600 + dil, res)
    rx, rw, rb, rr = tr.random_layer(n, h, w, 610 + dil, fp16=True)
    if res:
        truth = tr.truth_layer(rx, rw, rb, dil, res=rr)
        ok = lambda got: (bool(np.abs(got - truth).max() <= 1.2e-3 * np.abs(truth).max() + 1e-6),
                          f"max {tr.max_rel(got, truth):.2e} of max|ref| (bound 1.2e-3)")
    else:
        rr = None
        truth = tr.truth_layer(rx, rw, rb, dil, lrelu=False)
        scale = np.abs(truth).max()
        ok = lambda got: (bool(np.abs(got - tr.q16(truth)).max() <= 2e-3 * scale / 2 + 1e-6 and np.abs(got - truth).mean() < 3e-4 * scale),
                          f"max vs fp16(ref) {np.abs(got - tr.q16(truth)).max() / scale:.2e} mean {np.abs(got - truth).mean() / scale:.2e} of scale")
    _banded_sweep(eng16, f"k_ref_conv_f16_v2 dil {dil} tile {tw or 32} {'residual' if res else 'plain'} n={n} {h}x{w}",
                  lambda: eng16.dbg_ref_conv_f16(x, wt, b, dil, lrelu=True, residual=r, tile_w=tw), tr.layer_f16(x, wt, b, dil, r).astype(F32),
                  lambda: eng16.dbg_ref_conv_f16(rx, rw, rb, dil, lrelu=res, residual=rr, tile_w=tw), ok)


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("dil,h,w", [(1, 60, 130), (2, 60, 130), (4, 60, 70), (8, 60, 70)])
def test_split_layer_bands_at_small_grids(engx3, dil, h, w, n):
    """k_ref_conv_f16x3 (8 x 64 tiles at dilation 1 / 2, 8 x 32 at 4 / 8; one workgroup per CU: 24 tiles per image on 8 workgroups
    at cap 8), with the in-place residual.  Random family: max <= 6e-6 max|ref| (tests/test_gpu_f16.py::test_ref_conv_f16x3_layer)."""
    x, wt, b, r = tr.exact_x3_layer(n, 32, h, w, 700 + dil, res=True)
    rx, rw, rb, rr = tr.random_layer(n, h, w, 710 + dil)
    _banded_sweep(engx3, f"k_ref_conv_f16x3 dil {dil} residual n={n} {h}x{w}",
                  lambda: engx3.dbg_ref_conv_f16x3(x, wt, b, dil, lrelu=True, residual=r), tr.layer_x3(x, wt, b, dil, 1, r),
                  lambda: engx3.dbg_ref_conv_f16x3(rx, rw, rb, dil, lrelu=True, residual=rr), _rel(tr.truth_layer(rx, rw, rb, dil, res=rr), 6e-6))
    _banded_sweep(engx3, f"k_ref_conv_f16x3 dil {dil} plain n={n} {h}x{w}",
                  lambda: engx3.dbg_ref_conv_f16x3(x, wt, b, dil, lrelu=True), tr.layer_x3(x, wt, b, dil),
                  lambda: engx3.dbg_ref_conv_f16x3(rx, rw, rb, dil), _rel(tr.truth_layer(rx, rw, rb, dil, lrelu=False), 6e-6))


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("dil", [1, 2, 4, 8])
def test_f32_tower_layer_at_small_grids(eng32, dil, n):
    """k_ref_conv_f32 (one workgroup per CU over HALF tiles of 8 or 16 rows x 64 columns).  Random family: max < 2e-5 max|ref|
    (tests/test_gpu_fp32.py)."""
    h, w = 60, 132
    x, wt, b, r = tr.exact_f16_layer(n, h, w, 800 + dil, True)
    rx, rw, rb, rr = tr.random_layer(n, h, w, 810 + dil)
    _banded_sweep(eng32, f"k_ref_conv_f32 dil {dil} residual n={n} {h}x{w}",
                  lambda: eng32.dbg_conv2d(x, wt, b, 3, 1, dil, lrelu=True, residual=r, tower32=True), tr.layer_f32(x, wt, b, dil, r),
                  lambda: eng32.dbg_conv2d(rx, rw, rb, 3, 1, dil, lrelu=True, residual=rr, tower32=True),
                  _rel(tr.truth_layer(rx, rw, rb, dil, res=rr), 2e-5))


@pytest.mark.parametrize("split", [False, True], ids=["f16", "split"])
def test_refin_at_small_grids(eng16, engx3, split):
    """k_refin_f16, n = 2: 48 tiles of 8 x 64 on 16 workgroups at cap 8.  Random family (tests/test_gpu_f16.py::test_refin_f16_kernel):
    split: max <= 3e-6 scale + 1e-6; fp16: |got - fp16(ref)| <= 1e-3 scale and mean < 2e-4 scale, scale = max(1, max|ref|)."""
    eng = engx3 if split else eng16
    n, h, w = 2, 64, 144
    dl, in6, dmax, wt, b = tr.exact_refin(n, h, w, 900)
    v = tr.conv(tr.refin_input(dl, in6, dmax), wt, b)
    eref = tr.store_x3(v.astype(F32)) if split else tr.act16(v).astype(F32)
    rng = np.random.default_rng(901)
    rin = rng.integers(-128, 128, (n, 6, h, w), dtype=np.int8)
    rdl = (rng.random((n, h // 16, w // 16)) * 6.0).astype(F32)
    rw = (rng.standard_normal((32, 4, 3, 3)) / 4.0).astype(F32)
    rb = rng.standard_normal(32).astype(F32)
    truth = tr.lrelu64(tr.conv(tr.refin_input(rdl, rin, 96), rw, rb))
    scale = max(1.0, float(np.abs(truth).max()))
    if split:
        ok = lambda got: (bool(np.abs(got - truth).max() <= 3e-6 * scale + 1e-6), f"max {np.abs(got - truth).max() / scale:.2e} of scale")
    else:
        ok = lambda got: (bool(np.abs(got - tr.q16(truth)).max() <= 1e-3 * scale and np.abs(got - truth).mean() < 2e-4 * scale),
                          f"max vs fp16(ref) {np.abs(got - tr.q16(truth)).max() / scale:.2e} mean {np.abs(got - truth).mean() / scale:.2e} of scale")
    _banded_sweep(eng, f"k_refin_f16 {'split' if split else 'fp16'} n={n} {h}x{w}",
                  lambda: eng.dbg_refin(dl, in6, dmax, wt, b, split), eref, lambda: eng.dbg_refin(rdl, rin, 96, rw, rb, split), ok)


@pytest.mark.parametrize("dma", [False, True], ids=["k_conv_x3s", "k_feat_x3s_dma"])
@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
def test_lowres_3x3_at_small_grids(engx3, dma, res):
    """The 3x3 feature layers on split slots (8 x 16 tiles, two workgroups per CU; n = 2: 48 tiles on 16 workgroups at cap 8).
    Random family: max < 4e-6 max|ref| (tests/test_gpu_parity.py), and the zero-bordered kernel gives the plain one's bits."""
    n, h, w = 2, 60, 40
    x, wt, b, r = tr.exact_x3_layer(n, 32, h, w, 1000 + res, res=res)
    rx, rw, rb, rr = tr.random_layer(n, h, w, 1010 + res)
    rr = rr if res else None
    call = lambda a, k, c, q: engx3.dbg_conv2d(a, k, c, 3, 1, 1, lrelu=True, residual=q, x3=True, slots=True, dma=dma)
    _banded_sweep(engx3, f"{'k_feat_x3s_dma' if dma else 'k_conv_x3s 3x3'} {'residual' if res else 'plain'} n={n} {h}x{w}",
                  lambda: call(x, wt, b, r), tr.layer_x3(x, wt, b, 1, 1, r), lambda: call(rx, rw, rb, rr),
                  _rel(tr.truth_layer(rx, rw, rb, 1, res=rr), 4e-6),
                  (lambda: engx3.dbg_conv2d(rx, rw, rb, 3, 1, 1, lrelu=True, residual=rr, x3=True, slots=True)) if dma else None)


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("dma", [False, True], ids=["k_conv_x3s", "k_down_x3s_dma"])
def test_lowres_5x5_stride2_at_small_grids(engx3, dma, n):
    """The 5x5 stride-2 down-conv on split slots (4 x 32 tiles, or 4 x 16 for the zero-bordered kernel; one workgroup per CU).
    Random family: max < 4e-6 max|ref| (tests/test_gpu_parity.py)."""
    h, w = (64, 80) if dma else (64, 140)          # 32 x 40 or 32 x 70 outputs: 8 x 3 tiles either way
    x, wt, b, _ = tr.exact_x3_layer(n, 32, h, w, 1100, k=5, xmax=1)
    rx, rw, rb, _ = tr.random_layer(n, h, w, 1110, k=5)
    call = lambda a, k, c: engx3.dbg_conv2d(a, k, c, 5, 2, 1, lrelu=True, x3=True, slots=True, dma=dma)
    _banded_sweep(engx3, f"{'k_down_x3s_dma' if dma else 'k_conv_x3s 5x5'} n={n} {h}x{w}",
                  lambda: call(x, wt, b), tr.layer_x3(x, wt, b, 1, 2), lambda: call(rx, rw, rb), _rel(tr.truth_layer(rx, rw, rb, 1, 2), 4e-6),
                  (lambda: engx3.dbg_conv2d(rx, rw, rb, 5, 2, 1, lrelu=True, x3=True, slots=True)) if dma else None)


@pytest.mark.parametrize("dma", [False, True], ids=["k_conv_x3s", "k_agg_x3s_dma"])
def test_aggregation_layer_at_small_grids(engx3, dma):
    """The 3x3x3 layer on a volume of 4 planes of 20 x 40 (36 tiles of 8 x 16 on 8 workgroups at cap 8).  Random family: max < 4e-6
    max|ref| (tests/test_gpu_parity.py); the zero-bordered kernel gives the plain one's bits."""
    d, h, w = 4, 20, 40
    x, wt, b = tr.exact_x3_volume(d, h, w, 1200)
    rng = np.random.default_rng(1201)
    rx = rng.standard_normal((32, d, h, w)).astype(F32)
    rw = (rng.standard_normal((32, 32, 3, 3, 3)) / 30.0).astype(F32)
    rb = rng.standard_normal(32).astype(F32)
    call = lambda a, k, c: engx3.dbg_conv3d(a, k, c, lrelu=True, x3=True, slots=True, dma=dma)
    _banded_sweep(engx3, f"{'k_agg_x3s_dma' if dma else 'k_conv_x3s 3x3x3'} {d}x{h}x{w}",
                  lambda: call(x, wt, b), tr.layer3d_x3(x, wt, b), lambda: call(rx, rw, rb), _rel(tr.lrelu64(tr.conv3d(rx, rw, rb)), 4e-6),
                  (lambda: engx3.dbg_conv3d(rx, rw, rb, lrelu=True, x3=True, slots=True)) if dma else None)


def test_down0_at_small_grids(eng16):
    """k_down0_f16, two pairs = four eyes of 4 x 3 tiles (8 x 32) on 16 workgroups at cap 8.  Random family: max <= 2e-5 max(1,
    max|ref|) (tests/test_gpu_f16.py::test_down0_f16_kernel)."""
    n, h, w = 2, 64, 152
    in6, wt, b = tr.exact_down0(n, h, w, 1300)
    eref = np.concatenate([tr.store_x3(tr.down0(in6[i], wt, b).astype(F32), False) for i in range(n)])
    rng = np.random.default_rng(1301)
    rin = rng.integers(-128, 128, (n, 6, h, w), dtype=np.int8)
    rw = (rng.standard_normal((32, 3, 5, 5)) / 8.0).astype(F32)
    rb = rng.standard_normal(32).astype(F32)
    truth = np.concatenate([tr.down0(rin[i], rw, rb) for i in range(n)])
    scale = max(1.0, float(np.abs(truth).max()))
    _banded_sweep(eng16, f"k_down0_f16 n={n} pairs {h}x{w}", lambda: eng16.dbg_down0(in6, wt, b), eref, lambda: eng16.dbg_down0(rin, rw, rb),
                  lambda got: (bool(np.abs(got - truth).max() <= 2e-5 * scale), f"max {np.abs(got - truth).max() / scale:.2e} of scale"))


def test_down01_at_small_grids(eng16):
    """k_down01_f16 + k_down01_border, two pairs = four eyes of 2 x 3 tiles (8 x 32) on 8 workgroups at cap 8.  Random family: max <=
    3e-5 max(1, max|ref|) (tests/test_gpu_f16.py::test_down01_folded_kernels)."""
    n, h, w = 2, 64, 320
    in6, w0, b0, w1, b1 = tr.exact_down01(n, h, w, 1400)
    eref = np.concatenate([tr.store_x3(tr.down01(in6[i], w0, b0, w1, b1).astype(F32), False) for i in range(n)])
    rng = np.random.default_rng(1401)
    rin = rng.integers(-128, 128, (n, 6, h, w), dtype=np.int8)
    r0 = (rng.standard_normal((32, 3, 5, 5)) / 8.0).astype(F32)
    r1 = (rng.standard_normal((32, 32, 5, 5)) / 28.0).astype(F32)
    c0, c1 = rng.standard_normal(32).astype(F32), rng.standard_normal(32).astype(F32)
    truth = np.concatenate([tr.down01(rin[i], r0, c0, r1, c1) for i in range(n)])
    scale = max(1.0, float(np.abs(truth).max()))
    _banded_sweep(eng16, f"k_down01_f16 n={n} pairs {h}x{w}", lambda: eng16.dbg_down01(in6, w0, b0, w1, b1), eref,
                  lambda: eng16.dbg_down01(rin, r0, c0, r1, c1),
                  lambda got: (bool(np.abs(got - truth).max() <= 3e-5 * scale), f"max {np.abs(got - truth).max() / scale:.2e} of scale"))
