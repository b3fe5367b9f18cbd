"""The references of tests/golden/tower_ref.py on the CPU, before tests/test_gpu_tower_grids.py holds a kernel to them:
  * the float64 convolutions agree with the oracle and with torch float64;
  * every input of the exact family is exact: the operands bound every partial sum of every accumulator, in any order, to 24
    bits (budget), and summed forwards and backwards in float32 the result is the float64 one, bit for bit;
  * the reference outputs have no two equal rows in a channel (over images, row phases and strips), fewer than 1e-3 zeros and
    20 - 80 % negative values where a LeakyReLU (or the head's relu) ends the operation;
  * the criteria of the GPU test reject what a broken tile loop does to an output (tower_ref.MUTATIONS);
  * the sweep of the streamed blocks reaches every schedule transition it claims.
Runs without a GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tower_ref as tr

F32, F64 = np.float32, np.float64
T = lambda a: torch.from_numpy(np.ascontiguousarray(a, F64))


# ---- the convolutions ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,stride,dil", [(3, 1, 1), (3, 1, 2), (3, 1, 4), (3, 1, 8), (5, 2, 1)])
def test_conv_reference_is_the_oracle_and_torch(oracle, k, stride, dil):
    rng = np.random.default_rng(k + dil)
    x = rng.standard_normal((2, 32, 18, 22)).astype(F32)
    w = (rng.standard_normal((32, 32, k, k)) / 17.0).astype(F32)
    b = rng.standard_normal(32).astype(F32)
    got = tr.conv(x, w, b, dil, stride)
    ref = F.conv2d(T(x), T(w), T(b), stride=stride, padding=(k // 2) * dil, dilation=dil).numpy()
    assert got.shape == ref.shape and np.abs(got - ref).max() < 1e-12
    for i in range(2):
        o = oracle.conv2d(x[i], w, b, stride, (k // 2) * dil, dil)
        assert np.abs(got[i] - o).max() < 2e-5 * np.abs(o).max()
    for order in (0, 1):      # the explicit sequence of additions is the same sum
        assert np.abs(tr.conv_ordered(x, w, b, dil, stride, F64, order) - ref).max() < 1e-12


def test_conv3d_and_block_references_are_torch():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((32, 4, 9, 11)).astype(F32)
    w = (rng.standard_normal((32, 32, 3, 3, 3)) / 30.0).astype(F32)
    b = rng.standard_normal(32).astype(F32)
    ref = F.conv3d(T(x)[None], T(w), T(b), padding=1)[0].numpy()
    assert np.abs(tr.conv3d(x, w, b) - ref).max() < 1e-12
    bx, w1, b1, w2, b2 = tr.random_block(2, 11, 30, 4)
    t = F.leaky_relu(F.conv2d(T(bx), T(w1), T(b1), padding=2, dilation=2), float(F32(0.2)))
    y = F.leaky_relu(T(bx) + F.conv2d(t, T(w2), T(b2), padding=2, dilation=2), float(F32(0.2))).numpy()
    assert np.abs(tr.truth_block(bx, w1, b1, w2, b2, 2) - y).max() < 1e-12


def test_fp16_store_rule_and_the_split_pair():
    """act16 is act_pack2_f16 (round, then LeakyReLU on the fp16 value with the fp16 slope); the pair of a split value holds 22 bits"""
    v = np.array([3.0, -3.0, -1.0009765625, 1e-3, -65504.0, 0.0, -0.1], F64)
    h = v.astype(np.float16)
    want = np.maximum(h, (h * np.float16(0.2)).astype(np.float16)).astype(F64)      # numpy's fp16 product: one rounding of the exact product
    assert np.array_equal(tr.act16(v), want)
    assert tr.act16(np.array([-3.0]))[0] != np.float16(-0.6)                        # not LeakyReLU-then-round: -3 * 0.19995 = -0.59985
    x = (np.arange(-40, 41) / 8.0 + 2.0 ** -12).astype(F32)
    assert np.array_equal(tr.join(*tr.split(x)), x)


# ---- the exact family is exact -----------------------------------------------------------------------------------------------
def _f16_block_budgets(x, w1, b1, w2, b2, dil):
    t = tr.act16(tr.conv(x, w1, b1, dil))
    return t, max(tr.budget_conv(x, w1, b1, dil=dil), tr.budget_conv(t, w2, b2, res=x, dil=dil))


@pytest.mark.parametrize("n", tr.STREAM_N)
@pytest.mark.parametrize("dil,h,w", tr.STREAM_F16)
def test_exact_f16_block_and_its_conditions(dil, h, w, n):
    ops = tr.exact_f16_block(n, h, w, 100 + dil)
    t, bits = _f16_block_budgets(*ops, dil)
    assert bits <= 24 and t.min() > 0, (bits, t.min())          # conv1 stays positive: conv2's inputs are multiples of 1/8
    assert tr.grid_exp(t) >= -3
    tr.check_conditions(tr.block_f16(*ops, dil), tr.STREAM_OW_F16[dil], what="exact")
    rd = tr.random_block(n, h, w, 200 + dil, fp16=True)
    tr.check_conditions(tr.truth_block(*rd, dil, round_t=tr.q16), tr.STREAM_OW_F16[dil], what="random")


def test_exact_f16_block_in_two_summation_orders():
    """2 images of 13 x 70 at dilation 2, both convs summed forwards and backwards in float32: the float64 block, bit for bit"""
    x, w1, b1, w2, b2 = tr.exact_f16_block(2, 13, 70, 1)
    ref = tr.block_f16(x, w1, b1, w2, b2, 2)
    for order in (0, 1):
        t = tr.act16(tr.conv_ordered(x, w1, b1, 2, 1, F32, order))
        v = tr.conv_ordered(t, w2, b2, 2, 1, F32, order) + x          # float32: the residual add is exact as well
        assert v.dtype == F32 and tr.same_bits(tr.act16(v), ref), order
    c = tr.conditions(ref, 60)
    assert 0.4 < c["neg"] < 0.6 and c["zero"] < 1e-3 and c["dup"] == 0, c


@pytest.mark.parametrize("n", tr.STREAM_N)
@pytest.mark.parametrize("dil,h,w", tr.STREAM_X3)
def test_exact_split_block_and_its_conditions(dil, h, w, n):
    x, w1, b1, w2, b2 = tr.exact_x3_block(n, h, w, 300 + dil)
    assert tr.budget_x3(x, w1, b1, dil=dil) <= 24
    v1 = tr.sums_x3(x, w1, b1, lambda a, k: tr.conv(a, k, None, dil))
    t = tr.layer_x3(x, w1, b1, dil)
    assert v1.min() > 0 and np.array_equal(t.astype(F64), v1)          # the hi / lo pair holds conv1's sum exactly ...
    assert (tr.split(t)[1] != 0).mean() > 0.5 and (tr.split(x)[1] != 0).mean() > 0.3 and (tr.split(w1)[1] != 0).any()      # ... and lo parts are in play
    assert tr.budget_x3(t, w2, b2, res=x, dil=dil) <= 24
    tr.check_conditions(tr.block_x3(x, w1, b1, w2, b2, dil), tr.STREAM_OW_X3[dil], what="exact")
    tr.check_conditions(tr.truth_block(*tr.random_block(n, h, w, 400 + dil), dil), tr.STREAM_OW_X3[dil], what="random")


def test_exact_split_layer_in_two_summation_orders():
    """both accumulators of the split layer forwards and backwards in float32, then v = acc0 + acc1 / 2048 + residual in two
    orders of the additions: the float64 value, bit for bit"""
    x, w, b, r = tr.exact_x3_layer(2, 32, 13, 70, 3, res=True)
    assert (tr.split(x)[1] != 0).mean() > 0.3 and (tr.split(w)[1] != 0).mean() > 0.3 and tr.budget_x3(x, w, b, r, dil=2) <= 24
    (xh, xl), (wh, wl), (rh, rl) = tr.split(x), tr.split(w), tr.split(r)
    ref = tr.layer_x3(x, w, b, 2, 1, r)
    zero, inv = np.zeros(32, F32), F32(1.0 / 2048.0)
    for order in (0, 1):
        a0 = tr.conv_ordered(xh, wh, b if order == 0 else zero, 2, 1, F32, order)
        a1 = tr.conv_ordered(xh, wl, zero, 2, 1, F32, order)
        a1 = (a1 + tr.conv_ordered(xl, wh, zero, 2, 1, F32, order)).astype(F32) if order == 0 else \
            (tr.conv_ordered(xl, wh, zero, 2, 1, F32, order) + a1).astype(F32)
        if order == 0:
            v = ((a0 + a1 * inv) + (rh + rl * inv)).astype(F32)
        else:
            v = ((((rl * inv + a1 * inv) + rh) + a0) + b[None, :, None, None]).astype(F32)
        assert v.dtype == F32 and tr.same_bits(tr.store_x3(v), ref), order


# the banded cases of the GPU test: name -> (budget in bits, exact reference, strip / tile width, LeakyReLU at the end, random truth)
def _banded_cases():
    for dil, tw, h, w in [(1, 64, 60, 130), (1, 32, 60, 70), (2, 64, 60, 130), (2, 32, 60, 70), (4, 32, 60, 70), (8, 32, 60, 70)]:
        x, wt, b, r = tr.exact_f16_layer(2, h, w, 600 + dil, True)
        rx, rw, rb, rr = tr.random_layer(2, h, w, 610 + dil, fp16=True)
        yield f"f16 layer dil {dil} tw {tw}", tr.budget_conv(x, wt, b, r, dil=dil), tr.layer_f16(x, wt, b, dil, r), tw, True, tr.truth_layer(rx, rw, rb, dil, res=rr)
        x, wt, b, r = tr.exact_f16_layer(2, h, w, 600 + dil, False)
        yield f"f16 layer dil {dil} tw {tw} plain", tr.budget_conv(x, wt, b, dil=dil), tr.layer_f16(x, wt, b, dil), tw, True, None
    for dil, h, w in [(1, 60, 130), (2, 60, 130), (4, 60, 70), (8, 60, 70)]:
        for n in (1, 2):
            x, wt, b, r = tr.exact_x3_layer(n, 32, h, w, 700 + dil, res=True)
            rx, rw, rb, rr = tr.random_layer(n, h, w, 710 + dil)
            yield f"x3 layer dil {dil} n {n}", tr.budget_x3(x, wt, b, r, dil=dil), tr.layer_x3(x, wt, b, dil, 1, r), 64 if dil < 4 else 32, True, \
                tr.truth_layer(rx, rw, rb, dil, res=rr)
            yield f"x3 layer dil {dil} n {n} plain", tr.budget_x3(x, wt, b, dil=dil), tr.layer_x3(x, wt, b, dil), 64 if dil < 4 else 32, True, None
    for dil in (1, 2, 4, 8):
        x, wt, b, r = tr.exact_f16_layer(2, 60, 132, 800 + dil, True)
        yield f"f32 layer dil {dil}", tr.budget_conv(x, wt, b, r, dil=dil), tr.layer_f32(x, wt, b, dil, r), 64, True, None
    dl, in6, dmax, wt, b = tr.exact_refin(2, 64, 144, 900)
    x4 = tr.refin_input(dl, in6, dmax)
    v = tr.conv(x4, wt, b)
    assert np.array_equal(tr.join(*tr.split(x4[:, 0])).astype(F64), x4[:, 0]) and (tr.split(x4[:, 0])[1] != 0).any()      # d is a 22-bit pair
    yield "refin split", tr.budget_refin(x4, wt, b), tr.store_x3(v.astype(F32)), 64, True, None
    yield "refin f16", tr.budget_refin(x4, wt, b), tr.act16(v), 64, True, None
    for res in (False, True):
        x, wt, b, r = tr.exact_x3_layer(2, 32, 60, 40, 1000 + res, res=res)
        yield f"lowres 3x3 res {res}", tr.budget_x3(x, wt, b, r), tr.layer_x3(x, wt, b, 1, 1, r), 16, True, None
    for n in (1, 2):
        for h, w, tc in ((64, 80, 16), (64, 140, 32)):
            x, wt, b, _ = tr.exact_x3_layer(n, 32, h, w, 1100, k=5, xmax=1)
            yield f"lowres 5x5 n {n} {h}x{w}", tr.budget_x3(x, wt, b, stride=2), tr.layer_x3(x, wt, b, 1, 2), tc, True, None
    x, wt, b = tr.exact_x3_volume(4, 20, 40, 1200)
    yield "aggregation layer", tr.budget_x3(x, wt, b, conv_fn=tr.conv3d, caxis=0), tr.layer3d_x3(x, wt, b).transpose(1, 0, 2, 3), 16, True, None
    in6, wt, b = tr.exact_down0(2, 64, 152, 1300)
    xp = np.zeros((4, 3, 64, 160))
    xp[:, :, :, :152] = in6.reshape(4, 3, 64, 152) / 128.0
    yield "down0", tr.budget_x3(xp, wt, b, stride=2), tr.store_x3(tr.conv(xp, wt, b, 1, 2).astype(F32), False), 32, False, None
    in6, w0, b0, w1, b1 = tr.exact_down01(2, 64, 320, 1400)
    xa = np.abs(in6.reshape(4, 3, 64, 320) / 128.0)
    tot = tr.conv(tr.conv(xa, np.abs(w0), np.abs(b0), 1, 2), np.abs(w1), np.abs(b1), 1, 2)
    ref = np.concatenate([tr.down01(in6[i], w0, b0, w1, b1) for i in range(2)])
    assert np.array_equal(tr.store_x3(ref.astype(F32), False).astype(F64), ref)
    yield "down01", tr.budget(float(tot.max()), tr.grid_exp(xa) + tr.grid_exp(w0) + tr.grid_exp(w1)), ref, 32, False, None


def test_banded_exact_inputs_are_exact_and_meet_the_conditions():
    seen = 0
    for name, bits, ref, strip, lrelu, truth in _banded_cases():
        assert bits <= 24, (name, bits)
        tr.check_conditions(ref, strip, lrelu, what=name)
        if truth is not None:
            tr.check_conditions(truth, strip, lrelu, what=name + " random")
        seen += 1
    assert seen == 6 * 2 + 4 * 2 * 2 + 4 + 2 + 2 + 4 + 1 + 2


def test_down0_reference_is_the_split_layer_on_the_padded_eyes():
    in6, wt, b = tr.exact_down0(1, 20, 40, 5)
    xp = np.zeros((2, 3, 32, 48))
    xp[:, :, :20, :40] = in6.reshape(2, 3, 20, 40) / 128.0
    assert np.array_equal(tr.down0(in6[0], wt, b), tr.sums_x3(xp, wt, b, lambda a, k: tr.conv(a, k, None, 1, 2)))      # x has no lo part: x w exactly


@pytest.mark.parametrize("n", tr.STREAM_N)
def test_exact_tail_and_its_conditions(n):
    hk, wk, ho, wo, ups = tr.STREAM_TAIL
    x, w1, b1, w2, b2, hw, hb, low = ops = tr.exact_f16_tail(n, hk, wk, ups, 500)
    t, bits = _f16_block_budgets(x, w1, b1, w2, b2, 1)
    y = tr.block_f16(x, w1, b1, w2, b2, 1)
    assert bits <= 24 and t.min() > 0 and y.min() > 0 and tr.grid_exp(y) >= -6          # both convs positive: y on a grid of 2^-6
    assert np.array_equal(tr.q16(hw.astype(F32)), hw)                                    # head weights exact in fp16: no lo part
    assert tr.budget_conv(y, hw.reshape(1, 32, 3, 3), np.array([hb]), dil=1) <= 24
    out = tr.tail_f16(*ops, ups, 64.0, ho, wo)
    assert np.array_equal(out["disp"], np.maximum(out["pre"], 0)) and np.array_equal(out["disp"].astype(F32).astype(F64), out["disp"])
    tr.check_conditions(out["pre"][:, None], tr.STREAM_OW_TAIL, what="tail")            # 20 - 80 % negative: the relu clips those
    tr.check_conditions(y, tr.STREAM_OW_TAIL, lrelu=False, what="tail y")


# ---- what the criteria reject ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mut", tr.MUTATIONS)
def test_the_criteria_reject_a_broken_schedule(mut):
    """Bit equality with the exact reference, bit equality with the default grid's result (random family), and the bound of the
    default grid itself all reject every defect, at dilation 1 and 2, for the fp16 block, and for the split layer's tiles."""
    for dil, strip in ((1, 62), (2, 60)):
        ex = tr.block_f16(*tr.exact_f16_block(3, 13, 130, 7), dil).astype(F32)
        rd = tr.truth_block(*tr.random_block(3, 13, 130, 8, fp16=True), dil, round_t=tr.q16)
        for ref in (ex, rd.astype(F32)):
            bad = tr.mutate(ref, mut, dil, strip, (8, 64))
            assert not tr.same_bits(bad, ref), (mut, dil)
        bad = tr.mutate(rd, mut, dil, strip, (8, 64))
        err = np.abs(bad - rd)
        assert not (np.isfinite(bad).all() and err.max() <= 3e-3 * np.abs(rd).max()), (mut, dil)      # the fp16 block's bound
        assert not tr.within(bad, rd, 2e-5)                                                                # the split block's
    x, wt, b, r = tr.exact_x3_layer(2, 32, 20, 70, 9, res=True)
    ref = tr.layer_x3(x, wt, b, 1, 1, r)
    assert not tr.same_bits(tr.mutate(ref, mut, 1, 32, (8, 32)), ref)


def test_mutations_change_only_what_they_name():
    ref = tr.block_f16(*tr.exact_f16_block(2, 20, 130, 7), 1)
    for mut in tr.MUTATIONS:
        bad = tr.mutate(ref, mut, 1, 62, (8, 64))
        changed = ~((bad == ref) | (np.isnan(bad) & np.isnan(ref)))
        assert 0 < changed.mean() < 0.1, mut


# ---- the sweep reaches what it claims ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", tr.STREAM_N)
@pytest.mark.parametrize("kind", ["f16", "x3", "tail"])
def test_stream_sweep_reaches_every_transition(kind, n):
    cases = {"f16": [(d, h, w, tr.STREAM_OW_F16[d]) for d, h, w in tr.STREAM_F16],
             "x3": [(d, h, w, tr.STREAM_OW_X3[d]) for d, h, w in tr.STREAM_X3],
             "tail": [(1, tr.STREAM_TAIL[2], tr.STREAM_TAIL[3], tr.STREAM_OW_TAIL)]}[kind]
    for dil, h, w, ow in cases:
        s0 = tr.stream_sched(n, h, w, dil, ow, 256)
        assert s0["nstrips"] == 3 and w % ow and s0["hsub"] >= 5 and h <= 64 and w <= 320
        caps = tr.stream_caps(s0["total"], 256)
        scheds = [tr.stream_sched(n, h, w, dil, ow, c) for c in caps]
        assert caps[0] == 1 and scheds[0]["grid"] == 1 and scheds[0]["rpw"] == s0["total"]          # the whole launch in one workgroup
        assert len({s["rpw"] for s in scheds}) == len(caps) and scheds[-1]["rpw"] == max(1, -(-s0["total"] // 256))
        ev = set().union(*(tr.stream_events(s) for s in scheds))
        assert ev >= tr.STREAM_EVENTS - (set() if n > 1 else {"image_boundary"}), (kind, dil, ev)
        for s in scheds:          # the shares tile the flat sequence: every row once, in order
            flat = [(sp, v) for units in tr.stream_shares(s) for sp, v0, v1 in units for v in range(v0, v1)]
            assert flat == [(f // s["hsub"], f % s["hsub"]) for f in range(s["total"])]
