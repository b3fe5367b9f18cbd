"""The references of tests/golden/midstage_ref.py, proven on the CPU (no GPU): they agree with the C oracle and with torch in
float64, the inputs called exact really are (float32 in two summation orders and float64 give the same bits), and every
deliberate defect of midstage_ref.MUTATIONS is rejected by the criteria tests/test_gpu_midstage.py applies to the kernels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import midstage_ref as mr
import torch_ref
from hobot_stereonet_amd import confidence

F32, F64 = np.float32, np.float64


def _sam_sets():
    for s, (n, dl, hl, wl) in enumerate(mr.SAM_SHAPES):
        for r, regime in enumerate(mr.SAM_REGIMES):
            yield (n, dl, hl, wl), regime, mr.sam_inputs(n, dl, hl, wl, regime, 100 * s + r)


@pytest.fixture(scope="module")
def sam_sets():
    """every exact soft-argmin input set with its float32 cost (order 0) — computed once"""
    out = []
    for shape, regime, inp in _sam_sets():
        inp["cost"] = mr.contract(inp["vol"], inp["w"], inp["bias"], F32)
        out.append((shape, regime, inp))
    return out


# ---- 1. the references agree with the oracle ---------------------------------------------------------------------------
def test_cost_volume_against_the_oracle(oracle):
    any_sub = False
    for s, (n, dl, hl, wl) in enumerate(mr.SAM_SHAPES):
        f = mr.cost_features(n, hl, wl, dl, s)
        ref = mr.cost_volume(f, dl, F32)
        assert mr.same_bits(ref, mr.cost_volume(f, dl, F64).astype(F32))        # one subtraction: the float64 value rounds to it
        for i in range(n):
            o = oracle.cost_volume(f[2 * i], f[2 * i + 1], dl)                      # (c, dl, h, w)
            assert mr.same_bits(ref[i], np.ascontiguousarray(o.transpose(1, 0, 2, 3)))
            t = torch_ref.cost_volume(torch.from_numpy(f[2 * i][None]), torch.from_numpy(f[2 * i + 1][None]), dl)[0].numpy()
            assert mr.same_bits(ref[i], np.ascontiguousarray(t.transpose(1, 0, 2, 3)))
        val, sub = mr.split_twin(ref)
        assert np.abs(val.astype(F64) - ref).max() <= 2.0 ** -21 * np.abs(ref).max()      # 22 bits
        assert (ref == 0).mean() > 0.02 and (val[ref == 0] == 0).all()                   # the planted exact zeros
        any_sub = any_sub or bool(sub.any())
    assert any_sub                                                                       # the 2^-20 band reaches the fp16 subnormals


def test_contraction_shift_sum_and_soft_argmin_against_the_oracle(oracle, sam_sets):
    worst = 0.0
    for (n, dl, hl, wl), regime, inp in sam_sets:
        cost = inp["cost"]
        w5 = inp["w"].reshape(1, 32, 3, 3, 3)
        for i in range(n):
            o = oracle.conv3d(np.ascontiguousarray(inp["vol"][i].transpose(1, 0, 2, 3)), w5, np.array([inp["bias"]], F32))[0]
            assert mr.same_bits(o, cost[i]), (n, dl, hl, wl, regime)                     # integer work: exact
            od = oracle.soft_argmin(cost[i])
            e = mr.sam_disp_error(od[None], cost[i][None])
            worst = max(worst, e / mr.soft_argmin_bound(max(dl, 2)))
            assert e <= mr.soft_argmin_bound(dl), (n, dl, hl, wl, regime, e)
        t = torch_ref.soft_argmin(torch.from_numpy(cost.astype(F64)))
        assert np.abs(t.numpy() - mr.soft_argmin(cost)).max() <= 1e-12 * dl
        assert mr.same_bits(mr.shift_sum(inp["P"], inp["bias"], F32), cost)
        c1 = confidence.low(cost, mr.soft_argmin(cost).astype(F32))
        assert c1.min() >= 0.0 and c1.max() <= 1.0 + 1e-12 and (dl > 1 or (c1 == 1.0).all())
    print(f"oracle.soft_argmin on the exact costs: at most {worst:.2f} of the bound")


def test_upsample_against_the_oracle_and_torch(oracle):
    for s, (hk, wk, ho, wo, ups, n) in enumerate(mr.UPS_SHAPES):
        low = mr.upsample_lows(n, hk // ups, wk // ups, s)
        ref = mr.upsample(low, ups, hk, wk)
        t = F.interpolate(torch.from_numpy(low.astype(F64))[:, None], scale_factor=ups, mode="bilinear", align_corners=False)[:, 0]
        assert np.abs(t.numpy() * ups - ref).max() <= 1e-12 * ups * 11
        for i in range(n):
            o = oracle.upsample_bilinear(low[i], ups, float(ups))
            assert np.abs(o - ref[i]).max() <= mr.upsample_bound(low, ups)
        assert np.array_equal(mr.upsample(low, ups, ho, wo), ref[:, :ho, :wo])             # the crop is a crop


def test_head_against_the_oracle_and_torch(oracle):
    for s, (hk, wk, ho, wo, ups, n) in enumerate(mr.HEAD_SHAPES):
        x, w, b, low = mr.head_exact_inputs(n, hk, wk, ups, s)
        ref = mr.head(x, w, b, low, ups, 64.0, ho, wo, F32)
        for i in range(n):
            r = oracle.conv2d(x[i], w.reshape(1, 32, 3, 3), np.array([b], F32), 1, 1, 1)[0]
            assert mr.same_bits(np.maximum(F32(64.0) * r, F32(0))[:ho, :wo] + F32(0), ref["disp"][i] + F32(0))    # (+ 0: -0 == 0)
        rng = np.random.default_rng(s)
        xg = rng.standard_normal((n, 32, hk, wk))
        wg = rng.standard_normal((32, 9)) * 0.01
        lowg = mr.upsample_lows(n, hk // ups, wk // ups, s)
        got = mr.head(xg, wg, 0.003, lowg, ups, 96.0, ho, wo)
        acc = F.conv2d(torch.from_numpy(xg), torch.from_numpy(wg.reshape(1, 32, 3, 3)), torch.tensor([0.003], dtype=torch.float64), padding=1)[:, 0]
        up = F.interpolate(torch.from_numpy(lowg.astype(F64))[:, None], scale_factor=ups, mode="bilinear", align_corners=False)[:, 0] * ups
        t = torch.relu(up + 96.0 * acc)[:, :ho, :wo].numpy()
        assert np.abs(t - got["disp"]).max() <= 1e-11
        assert np.array_equal(got["raw"], np.rint(got["disp"].astype(F32) * mr.INV_Q).astype(np.int32))
        assert abs(got["mean_abs_dr"] - float((96.0 * acc[:, :ho, :wo]).abs().mean())) <= 1e-12


def test_pyramid_against_the_oracle_and_torch(oracle):
    for s, (n, h, w) in enumerate(mr.PYR_SHAPES):
        in6 = np.random.default_rng(s).integers(-128, 128, (n, 6, h, w)).astype(np.int8)
        ref32, ref64 = mr.pyramid(in6, 4, F32), mr.pyramid(in6, 4, F64)
        hp, wp = (h + 15) // 16 * 16, (w + 15) // 16 * 16
        img = np.zeros((n, 3, hp, wp), F32)
        img[:, :, :h, :w] = in6[:, :3].astype(F32) / F32(128)
        t = torch.from_numpy(img.astype(F64))
        for k in range(3):
            assert ref32[k].shape == (n, 3, hp >> (k + 1), wp >> (k + 1))
            assert np.array_equal(ref32[k].astype(F64), ref64[k])                          # exact: small integers over a power of two
            t = F.avg_pool2d(t, 2)
            assert np.array_equal(t.numpy(), ref64[k])
            img = np.stack([oracle.avgpool2(img[i]) for i in range(n)])
            assert mr.same_bits(img, ref32[k])


# ---- 2. the exact inputs really are exact --------------------------------------------------------------------------------
def test_exact_soft_argmin_inputs(sam_sets):
    for (n, dl, hl, wl), regime, inp in sam_sets:
        c0 = inp["cost"]
        c1 = mr.contract(inp["vol"], inp["w"], inp["bias"], F32, order=1)
        c64 = mr.contract(inp["vol"], inp["w"], inp["bias"], F64)
        assert mr.same_bits(c0, c1) and np.array_equal(c0.astype(F64), c64), (n, dl, hl, wl, regime)
        p1 = mr.shift_sum(inp["P"], inp["bias"], F32, order=1)
        assert mr.same_bits(c0, p1) and np.array_equal(mr.shift_sum(inp["P"], inp["bias"], F64), c64)
        assert np.array_equal(mr.partial_sums(inp["vol"], inp["w"]), inp["P"].astype(F64))     # P itself is exact in fp32
        assert np.abs(c64).max() < 2.0 ** 12 and np.array_equal(c64 * 16, np.rint(c64 * 16))
        spread = c64.max(1) - c64.min(1)
        if regime == "above40":
            assert c64.min() >= 40.0
        if regime == "below40":
            assert c64.max() <= -40.0
        if regime == "spread30" and dl > 2 and n * hl * wl >= 40:          # (the planted pixels are a minority)
            assert np.median(spread) > 10.0
        if regime == "spread1" and dl > 2 and n * hl * wl >= 40:
            assert np.median(spread) < 12.0
        for i, y, x, kind in inp["plants"]:            # a planted pixel holds exactly the planted costs
            c = c64[i, :, y, x]
            if kind == "far":
                assert np.abs(c).min() > 90.0
            elif dl > 1:
                lo = {"min_first": [0], "min_last": [dl - 1], "min_inner": [dl // 2], "two_minima": [0, dl - 1]}[kind]
                assert all(c[k] == c.min() for k in lo) and (np.delete(c, lo) == c.min() + 24.0).all()
        # the float32 twin of the kernel's soft-argmin meets the bound the kernel is held to
        assert mr.sam_disp_error(mr.soft_argmin(c0, F32), c0) <= mr.soft_argmin_bound(dl), (n, dl, hl, wl, regime)


def test_exact_head_inputs():
    for s, (hk, wk, ho, wo, ups, n) in enumerate(mr.HEAD_SHAPES):
        x, w, b, low = mr.head_exact_inputs(n, hk, wk, ups, s)
        a = mr.head(x, w, b, low, ups, 64.0, ho, wo, F32, order=0)
        c = mr.head(x, w, b, low, ups, 64.0, ho, wo, F32, order=1)
        t = mr.head(x, w, b, low, ups, 64.0, ho, wo, F64)
        assert mr.same_bits(a["disp"] + F32(0), c["disp"] + F32(0)) and np.array_equal(a["disp"].astype(F64), t["disp"])
        assert np.array_equal(a["raw"], t["raw"]) and abs(a["mean_abs_dr"] - t["mean_abs_dr"]) == 0.0
        assert (t["disp"] == 0).any() and t["disp"].std() > 0.5                              # the relu clips, the map is not constant
        # the split form's operands: weights exact in fp16 (lo part zero), x = hi + lo / 2048 exactly with a non-zero lo somewhere
        assert np.array_equal(w.astype(np.float16).astype(F32), w)
        hi = x.astype(np.float16).astype(F32)
        lo = ((x - hi) * F32(2048)).astype(np.float16).astype(F32)
        assert np.array_equal(hi + lo * F32(1 / 2048), x) and (lo != 0).any()


# ---- 3. the inputs discriminate ---------------------------------------------------------------------------------------------
def _rejected(mut, sam_sets):
    """True when the criterion of tests/test_gpu_midstage.py rejects the mutant on at least one of the chosen input sets"""
    if mut in ("mask_gt", "right_plus1"):
        for s, (n, dl, hl, wl) in enumerate(mr.SAM_SHAPES):
            f = mr.cost_features(n, hl, wl, dl, s)
            good, bad = mr.split_twin(mr.cost_volume(f, dl, F32))[0], mr.split_twin(mr.cost_volume(f, dl, F32, mut))[0]
            if not mr.same_bits(good, bad):
                return True
    if mut in ("drop_last_plane", "dz_swapped", "batch_wrap"):
        return any(not mr.same_bits(inp["cost"], mr.contract(inp["vol"], inp["w"], inp["bias"], F32, mut=mut)) for _, _, inp in sam_sets)
    if mut in ("extra_zero_plane", "no_max_subtraction"):
        return any(mr.sam_disp_error(mr.soft_argmin(inp["cost"], F32, mut), inp["cost"]) > mr.soft_argmin_bound(shape[1])
                   for shape, _, inp in sam_sets)
    if mut in ("crop_edge_pad", "col62_from_61"):
        for s, (hk, wk, ho, wo, ups, n) in enumerate(mr.HEAD_SHAPES):
            x, w, b, low = mr.head_exact_inputs(n, hk, wk, ups, s)
            if not mr.same_bits(mr.head(x, w, b, low, ups, 64.0, ho, wo, F32)["disp"], mr.head(x, w, b, low, ups, 64.0, ho, wo, F32, mut=mut)["disp"]):
                return True
    if mut in ("no_edge_clamp", "align_corners"):
        for s, (hk, wk, ho, wo, ups, n) in enumerate(mr.UPS_SHAPES):
            low = mr.upsample_lows(n, hk // ups, wk // ups, s)
            bad = np.maximum(mr.upsample(low, ups, ho, wo, F32, mut), 0)
            if np.abs(bad - mr.upsample(low, ups, ho, wo)).max() > mr.upsample_bound(low, ups):
                return True
    return False


@pytest.mark.parametrize("mut", mr.MUTATIONS)
def test_the_inputs_reject_the_mutant(mut, sam_sets):
    assert _rejected(mut, sam_sets), mut


def test_the_unmutated_twins_pass_every_criterion():
    for s, (hk, wk, ho, wo, ups, n) in enumerate(mr.UPS_SHAPES):
        low = mr.upsample_lows(n, hk // ups, wk // ups, s)
        assert np.abs(np.maximum(mr.upsample(low, ups, ho, wo, F32), 0) - mr.upsample(low, ups, ho, wo)).max() <= mr.upsample_bound(low, ups)
