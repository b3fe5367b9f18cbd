"""The kernels between the feature tower and the output maps, one at a time, through the sn_dbg_* mid-stage hooks (cost volume,
fp32 first aggregation layer, aggregation tail, soft-argmin, refinement heads, image pyramid) against the references of
tests/golden/midstage_ref.py.  tests/test_midstage_refs.py proves on the CPU that those references agree with the oracle, that
the inputs called exact are exact, and that the criteria used here reject an off-by-one mask, a swapped dz tap, a stray plane,
a missing max-subtraction, a wrapped pixel index, a crop-edge tap, an unclamped upsample and a copied tile column.
Every hook pre-fills its outputs with the 0xff pattern, so an unwritten element reads back as NaN (int32: -1), and checks guard
bands around them.  Needs an MI355X.  The lines starting with `midstage` are the record in profiles/midstage_parity.txt."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import midstage_ref as mr
import truth_compare as tc
from hobot_stereonet_amd import api, confidence
from test_gpu_confidence import LOW_TOL
from test_gpu_tail import _operands

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
sid = lambda t: "-".join(str(v) for v in t)


@pytest.fixture(scope="module")
def eng32(model_factory):
    eng = api.StereoNetHIP(model_factory(96, 64, 48), max_batch=2, precision=api.PREC_FP32)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def eng16(model_factory):
    eng = api.StereoNetHIP(model_factory(96, 64, 48), max_batch=2, precision=api.PREC_F16X3)
    yield eng
    eng.close()


def lrelu(v):
    return np.where(v > 0, v, v * v.dtype.type(0.2))


# ---- cost volume ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mr.SAM_SHAPES, ids=sid)
def test_cost_volume_is_the_twin_bit_for_bit(eng32, shape):
    """k_cost_slots and k_cost_slots_pad against v = fl - fr, hi = fp16(v), lo = fp16((v - hi) 2048), hi + lo / 2048 in float32."""
    n, dl, hl, wl = shape
    f = mr.cost_features(n, hl, wl, dl, mr.SAM_SHAPES.index(shape))
    ref, sub = mr.split_twin(mr.cost_volume(f, dl, F32))
    g0, g1 = eng32.dbg_cost_volume(f, dl, 0), eng32.dbg_cost_volume(f, dl, 1)       # (form 1: the hook checked the zero borders)
    diff = mr.bits(g0) != mr.bits(ref)
    print(f"midstage cost_volume {sid(shape)}: {int(diff.sum())} of {diff.size} values differ from the twin "
          f"({int((diff & sub).sum())} of them where hi or lo is an fp16 subnormal; {int(sub.sum())} such values), "
          f"max |diff| {float(np.abs(g0.astype(F64) - ref).max()):.3e}")
    assert np.isfinite(g0).all() and np.isfinite(g1).all()                            # every element written
    assert mr.same_bits(g0, g1)
    assert mr.same_bits(g0, ref)


# ---- the fp32 first aggregation layer (cost volume in the loader) ------------------------------------------------------
@pytest.mark.parametrize("shape", mr.SAM_SHAPES, ids=sid)
def test_agg_first_f32_against_the_oracle(eng32, oracle, shape):
    n, dl, hl, wl = shape
    rng = np.random.default_rng(sum(shape))
    f = mr.cost_features(n, hl, wl, dl, 50 + mr.SAM_SHAPES.index(shape))
    wt = (rng.standard_normal((32, 32, 3, 3, 3)) / 30.0).astype(F32)
    b = rng.standard_normal(32).astype(F32)
    got = eng32.dbg_agg_first_f32(f, dl, wt, b)
    assert np.isfinite(got).all()
    worst = 0.0
    for i in range(n):
        ref = lrelu(oracle.conv3d(oracle.cost_volume(f[2 * i], f[2 * i + 1], dl), wt, b))
        worst = max(worst, float(np.abs(got[i] - ref).max() / (np.abs(ref).max() + 1e-12)))
    print(f"midstage agg_first_f32 {sid(shape)}: max rel err {worst:.2e} (bound 2e-5)")
    assert worst < 2e-5


# ---- soft-argmin, exact inputs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mr.SAM_SHAPES, ids=sid)
def test_softargmin_exact_inputs(eng32, oracle, shape):
    """Both soft-argmin kernels on costs that are exact in fp32 (small integers, power-of-two weights; the CPU test proves it), in
    four regimes: spread about 1, about 30, all costs >= +40, all <= -40, with planted one-hot and double minima.
    cost: bit-equal to the reference, both forms, with and without the confidence plane, which must change neither cost nor
    disp_low.  disp_low: within (Dl - 1)(Dl + 4) 2^-23 planes of the float64 soft-argmin of those costs — the weights sum to one;
    each carries one rounded subtraction, one expf and at most Dl additions, the quotient one more rounding, times the largest
    plane index; a factor of two is slack.  conf_low: confidence.low of the kernel's own cost and disp_low within LOW_TOL, exactly
    1 at Dl = 1."""
    n, dl, hl, wl = shape
    s = mr.SAM_SHAPES.index(shape)
    worst_d = worst_o = worst_c = 0.0
    for r, regime in enumerate(mr.SAM_REGIMES):
        inp = mr.sam_inputs(n, dl, hl, wl, regime, 100 * s + r)
        cost = mr.contract(inp["vol"], inp["w"], inp["bias"], F32)
        truth = mr.soft_argmin(cost.astype(F64))
        worst_o = max(worst_o, max(float(np.abs(oracle.soft_argmin(cost[i]) - truth[i]).max()) for i in range(n)))
        first = None
        for form, v, w in ((0, inp["vol"], inp["w"]), (1, inp["P"], None)):
            for want_conf in (False, True):
                tag = f"{regime} form {form} conf {want_conf}"
                out = eng32.dbg_softargmin(v, inp["bias"], w, want_conf)
                assert out["nonfinite"] == 0, tag
                assert mr.same_bits(out["cost"], cost), tag
                assert np.isfinite(out["disp_low"]).all(), tag
                e = mr.sam_disp_error(out["disp_low"], cost)
                worst_d = max(worst_d, e)
                assert e <= mr.soft_argmin_bound(dl), (tag, e)
                if first is None:
                    first = out
                assert mr.same_bits(out["disp_low"], first["disp_low"]), tag           # neither the form nor the plane changes it
                if want_conf:
                    c = out["conf_low"]
                    ec = float(np.abs(c - confidence.low(out["cost"], out["disp_low"])).max())
                    worst_c = max(worst_c, ec)
                    assert ec <= LOW_TOL, (tag, ec)
                    assert dl > 1 or (c == F32(1.0)).all(), tag
                else:
                    assert np.isnan(out["conf_low"]).all(), tag                           # not asked for: not touched
    print(f"midstage softargmin {sid(shape)}: max |disp_low - truth| {worst_d:.3e} planes (bound {mr.soft_argmin_bound(dl):.3e}; "
          f"oracle.soft_argmin on the same costs {worst_o:.3e}), max |conf_low - twin| {worst_c:.3e}")


@pytest.mark.parametrize("shape", [s for s in mr.SAM_SHAPES if s[0] * s[2] * s[3] >= 15], ids=sid)
def test_softargmin_counts_nonfinite_pixels(eng32, shape):
    """+inf, -inf and NaN planted in a second input set: two planes of one pixel, and (n > 1) the last pixel of an image and the
    first of the next.  k_softargmin_p reads every P element for exactly one (plane, pixel), so the count is the number of
    planted pixels; k_head_softargmin multiplies a planted volume element into the 27 outputs around it (0 x inf is NaN), so
    there it is the number of pixels in the 3 x 3 neighbourhoods.  Every other pixel is bit-equal to the run without the plants."""
    n, dl, hl, wl = shape
    inp = mr.sam_inputs(n, dl, hl, wl, "spread30", 900 + mr.SAM_SHAPES.index(shape))
    npix = n * hl * wl
    pix = [npix // 3, npix - 1, 0] + ([hl * wl - 1, hl * wl] if n > 1 else [])
    vals = [np.inf, -np.inf, np.nan, np.inf, np.nan]
    for form, key, centre in ((0, "vol", 0), (1, "P", 13)):
        clean = eng32.dbg_softargmin(inp[key], inp["bias"], inp["w"] if form == 0 else None, True)
        v = inp[key].copy()
        bad = np.zeros((n, hl, wl), bool)
        for p, val in zip(pix, vals):
            i, y, x = p // (hl * wl), (p % (hl * wl)) // wl, p % wl
            v[i, 0, centre, y, x] = val
            if p == pix[0]:
                v[i, dl - 1, centre, y, x] = -val                          # a second plane of the same pixel
            bad[i, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] |= form == 0
            bad[i, y, x] = True
        out = eng32.dbg_softargmin(v, inp["bias"], inp["w"] if form == 0 else None, True)
        k = int(bad.sum())
        print(f"midstage nonfinite {sid(shape)} form {form}: count {out['nonfinite']} (expected {k})")
        assert out["nonfinite"] == k and clean["nonfinite"] == 0
        assert np.array_equal(~np.isfinite(out["cost"]).all(1), bad)
        keep = ~bad
        for name in ("disp_low", "conf_low"):
            assert np.array_equal(mr.bits(out[name])[keep], mr.bits(clean[name])[keep]), (form, name)
        assert np.array_equal(mr.bits(out["cost"])[np.broadcast_to(keep[:, None], out["cost"].shape)],
                              mr.bits(clean["cost"])[np.broadcast_to(keep[:, None], out["cost"].shape)])


# ---- the last aggregation layer in its fp32-output forms + soft-argmin ---------------------------------------------------
@pytest.mark.parametrize("gain", [1.0, 16.0], ids=["agg.out", "agg.out-x16"])
@pytest.mark.parametrize("shape", mr.TAIL_SHAPES, ids=sid)
def test_agg_tail_forms(eng16, oracle, shape, gain):
    """Forms 0 (plain slots, k_conv_x3s with fp32 output) and 1 (zero-bordered, k_agg_x3s_dma<false>) run the same MFMAs in the
    same order: volume, cost, disp_low and conf_low bit-equal.  Forms 1 and 2 (partial sums P + k_softargmin_p) against the
    float64 truth: mean and max error of cost and disp_low at most X3_FACTOR times the fp32 oracle path's on the same operands."""
    n, dl, hl, wl = shape
    rng = np.random.default_rng(dl + hl + wl)
    x = rng.standard_normal((n, 32, dl, hl, wl)).astype(F32)
    wt = (rng.standard_normal((32, 32, 3, 3, 3)) / 30.0).astype(F32)
    b = rng.standard_normal(32).astype(F32)
    ow = (rng.standard_normal((32, 27)) / 30.0 * gain).astype(F32)
    ob = F32(rng.standard_normal() * 0.1 * gain)
    y64 = F.conv3d(torch.from_numpy(x.astype(F64)), torch.from_numpy(wt.astype(F64)), torch.from_numpy(b.astype(F64)), padding=1)
    y64 = lrelu(y64.numpy())                                                       # (n, 32, dl, hl, wl)
    t_cost = mr.contract(y64.transpose(0, 2, 1, 3, 4), ow, ob)
    t_disp = mr.soft_argmin(t_cost)
    o_cost = np.stack([oracle.conv3d(lrelu(oracle.conv3d(x[i], wt, b)), ow.reshape(1, 32, 3, 3, 3), np.array([ob], F32))[0] for i in range(n)])
    o_disp = np.stack([oracle.soft_argmin(o_cost[i]) for i in range(n)])
    ref = {"cost": tc.err(o_cost, t_cost)[:2], "disp_low": tc.err(o_disp, t_disp)[:2]}
    out = [eng16.dbg_agg_tail(x, wt, b, ow, ob, form, want_conf=True) for form in (0, 1, 2)]
    for o in out:
        assert o["nonfinite"] == 0 and all(np.isfinite(o[k]).all() for k in ("cost", "disp_low", "conf_low"))
    for form in (1, 2):
        for k, truth in (("cost", t_cost), ("disp_low", t_disp)):
            e = tc.err(out[form][k], truth)
            print(f"midstage agg_tail {sid(shape)} gain {gain:g} form {form} {k}: mean/max {tc.fmt(e[:2])} (oracle path {tc.fmt(ref[k])})")
    for k in ("layer_vol", "cost", "disp_low", "conf_low"):
        assert mr.same_bits(out[0][k], out[1][k]), k
    assert tc.err(out[1]["layer_vol"], y64)[1] <= 1e-5 * np.abs(y64).max()             # and it is the layer
    for form in (1, 2):
        for k, truth in (("cost", t_cost), ("disp_low", t_disp)):
            assert not tc.stage_failures(out[form][k], truth, ref[k], tc.X3_FACTOR), (form, k)


# ---- refinement heads ----------------------------------------------------------------------------------------------------------
def _heads(eng32, eng16, *args):
    """forms 0, 1 (fp32 engine) and 2 (fp16-mode engine)"""
    return [eng32.dbg_head(*args, form=0), eng32.dbg_head(*args, form=1), eng16.dbg_head(*args, form=2)]


@pytest.mark.parametrize("shape", mr.HEAD_SHAPES, ids=sid)
def test_head_exact_inputs(eng32, eng16, shape):
    """Small-integer activations (with a non-zero fp16 lo part), head weights and bias multiples of 2^-6, dnorm 64, low = 0: every
    partial sum is exact in fp32, so k_head_final, k_head_final_mfma32 and k_head_final_f16<true> must give the reference's bits."""
    hk, wk, ho, wo, ups, n = shape
    x, w, b, low = mr.head_exact_inputs(n, hk, wk, ups, mr.HEAD_SHAPES.index(shape))
    ref = mr.head(x, w, b, low, ups, 64.0, ho, wo, F32)
    mean64 = mr.head(x, w, b, low, ups, 64.0, ho, wo, F64)["mean_abs_dr"]
    assert (ref["disp"] == 0).any() and ref["disp"].std() > 0.5                       # the relu clips, the map is not constant
    for form, o in enumerate(_heads(eng32, eng16, x, w, b, low, ups, 64.0, ho, wo)):
        assert np.isfinite(o["disp"]).all() and (o["raw"] >= 0).all(), form           # every pixel written
        bad = np.argwhere(mr.bits(o["disp"]) != mr.bits(ref["disp"]))
        assert bad.size == 0, f"form {form}: {len(bad)} pixels differ, first at (image, row, column) {bad[0]}"
        assert np.array_equal(o["raw"], ref["raw"]) and np.array_equal(o["raw"], np.rint(o["disp"] * mr.INV_Q).astype(np.int32)), form
        assert o["nonfinite"] == 0, form
        print(f"midstage head_exact {sid(shape)} form {form}: bit-equal; mean |D r| {o['mean_abs_dr']:.7f} (float64 {mean64:.7f})")
        assert abs(o["mean_abs_dr"] - mean64) <= 1e-4, form


@pytest.mark.parametrize("shape", mr.UPS_SHAPES, ids=sid)
def test_head_upsample_only(eng32, eng16, shape):
    """x = 0 and bias 0: disp = relu(up).  Against the float64 half-pixel bilinear upsample with edge clamp: at most
    6 x 2^-24 x max |low| x factor (the roundings of upsample_map's expression).  1 x N and N x 1 low maps included."""
    hk, wk, ho, wo, ups, n = shape
    low = mr.upsample_lows(n, hk // ups, wk // ups, mr.UPS_SHAPES.index(shape))
    x = np.zeros((n, 32, hk, wk), F32)
    w = mr.head_exact_inputs(1, 16, 16, 16, 0)[1]
    ref = mr.upsample(low, ups, ho, wo)
    for form, o in enumerate(_heads(eng32, eng16, x, w, 0.0, low, ups, 64.0, ho, wo)):
        e = float(np.abs(o["disp"] - ref).max())
        print(f"midstage head_upsample {sid(shape)} low {low.shape[1]}x{low.shape[2]} form {form}: max err {e:.3e} (bound {mr.upsample_bound(low, ups):.3e})")
        assert np.isfinite(o["disp"]).all() and e <= mr.upsample_bound(low, ups), form
        assert o["mean_abs_dr"] == 0.0 and o["nonfinite"] == 0, form


@pytest.mark.parametrize("shape", mr.HEAD_SHAPES, ids=sid)
def test_head_general_inputs(eng32, eng16, oracle, shape):
    """The operands of test_gpu_tail: forms 0 and 1 within FP32_FACTOR, form 2 within X3_FACTOR of the fp32 oracle path's own error
    (oracle.conv2d, oracle.upsample_bilinear, relu) against the float64 reference, mean and max."""
    hk, wk, ho, wo, ups, n = shape
    x, _, _, _, _, hw, hb, low = _operands(hk * 13 + wk + ups, n, hk, wk, ups)
    dnorm = 192.0 if ups == 16 else 96.0
    truth = mr.head(x, hw, hb, low, ups, dnorm, ho, wo)["disp"]
    orc = np.stack([np.maximum(oracle.upsample_bilinear(low[i], ups, float(ups))[:hk, :wk] +
                               F32(dnorm) * oracle.conv2d(x[i], hw.reshape(1, 32, 3, 3), np.array([hb], F32), 1, 1, 1)[0], 0)[:ho, :wo]
                    for i in range(n)])
    ref = tc.err(orc, truth)[:2]
    outs = _heads(eng32, eng16, x, hw, hb, low, ups, dnorm, ho, wo)
    for form, o in enumerate(outs):
        print(f"midstage head_general {sid(shape)} form {form}: mean/max {tc.fmt(tc.err(o['disp'], truth)[:2])} (oracle path {tc.fmt(ref)})")
    for form, o in enumerate(outs):
        assert o["nonfinite"] == 0 and (o["raw"] >= 0).all()
        assert not tc.stage_failures(o["disp"], truth, ref, tc.FP32_FACTOR if form < 2 else tc.X3_FACTOR), form
        assert np.array_equal(o["raw"], np.rint(o["disp"] * mr.INV_Q).astype(np.int32)), form


def test_head_forms_need_their_engine(eng32, eng16):
    x, w, b, low = mr.head_exact_inputs(1, 16, 16, 16, 0)
    for eng, form in ((eng32, 2), (eng16, 0), (eng16, 1)):
        with pytest.raises(api.StereoNetError) as ei:
            eng.dbg_head(x, w, b, low, 16, 64.0, 16, 16, form=form)
        assert "SN_PREC_FP32" in str(ei.value) or "fp16 mode" in str(ei.value)
    assert eng32.dbg_head(x, w, b, low, 16, 64.0, 16, 16, form=0)["nonfinite"] == 0      # the handles stay usable


# ---- image pyramid -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mr.PYR_SHAPES, ids=sid)
def test_pyramid_is_exact(eng32, oracle, shape):
    n, h, w = shape
    in6 = np.random.default_rng(mr.PYR_SHAPES.index(shape)).integers(-128, 128, (n, 6, h, w)).astype(np.int8)
    ref = mr.pyramid(in6, 4, F32)
    got = eng32.dbg_img_pool2(in6, 4)
    hp, wp = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    img = np.zeros((n, 3, hp, wp), F32)
    img[:, :, :h, :w] = in6[:, :3].astype(F32) / F32(128)
    for k in range(3):
        img = np.stack([oracle.avgpool2(img[i]) for i in range(n)])
        assert mr.same_bits(got[k], ref[k]) and mr.same_bits(got[k], img), k
    print(f"midstage pyramid {sid(shape)}: levels 1-3 bit-equal to the reference and to oracle.avgpool2")
