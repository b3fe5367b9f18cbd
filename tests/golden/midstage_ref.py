"""References for the kernels between the feature tower and the output maps (tests/test_midstage_refs.py proves them on the
CPU, tests/test_gpu_midstage.py holds the sn_dbg_* mid-stage hooks to them): cost volume and its hi / lo split, the 3x3x3
32 -> 1 contraction, the 27-shift sum over the partial sums P, soft-argmin, the refinement head (3x3 conv zero-padded at the
TENSOR edge, half-pixel bilinear upsample with edge clamp, relu, wire rounding) and the 2x2 pooling of the image pyramid.

Everything is numpy.  `dtype` selects float64 (the truth) or float32 (a twin of the kernel's arithmetic where the inputs are
exact: every partial sum representable, so the summation order cannot matter — `order` picks one of two orders so that a test
can show it does not).  `mut` names ONE deliberate defect (MUTATIONS); the input generators below are chosen so that the
criteria of tests/test_gpu_midstage.py reject every one of them, which the CPU test asserts.
"""
from __future__ import annotations

import numpy as np

from hobot_stereonet_amd import spec

MUTATIONS = ("mask_gt", "right_plus1", "drop_last_plane", "dz_swapped", "extra_zero_plane", "no_max_subtraction", "batch_wrap",
             "crop_edge_pad", "no_edge_clamp", "align_corners", "col62_from_61")
SPLIT = np.float32(2048.0)
F16_MIN_NORMAL = 2.0 ** -14


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 2: np.uint16}[a.dtype.itemsize])


# ---- cost volume ---------------------------------------------------------------------------------------------------------
def cost_volume(feat, dl, dtype=np.float64, mut=None):
    """feat (2n, 32, h, w), left / right interleaved -> (n, dl, 32, h, w): x >= d ? fl[x] - fr[x - d] : 0"""
    f = np.asarray(feat, dtype)
    n, h, w = f.shape[0] // 2, f.shape[2], f.shape[3]
    fl, fr = f[0::2], f[1::2]
    out = np.zeros((n, dl, 32, h, w), dtype)
    for d in range(dl):
        first = d + 1 if mut == "mask_gt" else d                 # first column with a value
        shift = d - 1 if mut == "right_plus1" else d             # right-eye column = x - shift
        for x in range(first, w):
            xr = x - shift
            if 0 <= xr < w:
                out[:, d, :, :, x] = fl[:, :, :, x] - fr[:, :, :, xr]
            else:                                                # (only the mutant reads past the row: the next element in memory)
                flat = fr.reshape(n, 32, h * w)
                idx = np.arange(h) * w + xr
                out[:, d, :, :, x] = fl[:, :, :, x] - flat[:, :, np.clip(idx, 0, h * w - 1)]
    return out


def split_twin(v):
    """float32 twin of the split-slot round trip: hi = fp16(v), lo = fp16((v - hi) 2048), value = hi + lo / 2048.
    -> (value float32, subnormal mask: hi or lo is a non-zero fp16 subnormal)"""
    v = np.asarray(v, np.float32)
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float32)) * SPLIT).astype(np.float16)
    val = hi.astype(np.float32) + lo.astype(np.float32) * np.float32(1.0 / 2048.0)
    sub = lambda a: (a != 0) & (np.abs(a.astype(np.float32)) < F16_MIN_NORMAL)
    return val, sub(hi) | sub(lo)


def cost_features(n, hl, wl, dl, seed):
    """Standard-normal features; in some rows the right eye is the left eye shifted by a disparity d < dl (exact zeros in plane
    d), and one band of channels is scaled down to magnitudes around 2^-20."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((2 * n, 32, hl, wl)).astype(np.float32)
    for i in range(n):
        for y in range(0, hl, 2):
            d = (y // 2 + i) % dl
            if d < wl:
                f[2 * i + 1, :, y, : wl - d] = f[2 * i, :, y, d:]
    f[:, 24:28] *= np.float32(2.0 ** -10)
    f[:, 28:32] *= np.float32(2.0 ** -20)
    return f


# ---- 3x3x3 32 -> 1 contraction, and the same cost from the partial sums P ----------------------------------------------
def _pad3(a):          # (n, dl, ..., h, w): one zero plane / row / column on both sides
    pw = [(0, 0)] * a.ndim
    pw[1] = pw[-2] = pw[-1] = (1, 1)
    return np.pad(a, pw)


def contract(vol, w, bias, dtype=np.float64, order=0, mut=None):
    """vol (n, dl, 32, h, w), w (32, 27) with tap = dz 9 + ky 3 + kx -> cost (n, dl, h, w), zero padding in d, y and x"""
    v = np.asarray(vol, dtype)
    n, dl, _, h, wd = v.shape
    if mut == "drop_last_plane":
        v = v.copy()
        v[:, dl - 1] = 0
    if mut == "batch_wrap":          # the batch as ONE tall image: the rows of neighbouring images are each other's padding
        v = v.transpose(1, 2, 0, 3, 4).reshape(1, dl, 32, n * h, wd)
    p = _pad3(v)
    hh = v.shape[3]
    wt = np.asarray(w, dtype).reshape(32, 27)
    acc = np.full((v.shape[0], dl, hh, wd), dtype(bias), dtype)
    pairs = [(c, t) for c in range(32) for t in range(27)]
    if order == 1:
        pairs = [(c, t) for t in reversed(range(27)) for c in reversed(range(32))]
    for c, t in pairs:
        dz, ky, kx = t // 9, (t // 3) % 3, t % 3
        if mut == "dz_swapped":
            dz = 2 - dz
        if wt[c, t] != 0:
            acc = acc + wt[c, t] * p[:, dz:dz + dl, c, ky:ky + hh, kx:kx + wd]
    if mut == "batch_wrap":
        acc = acc.reshape(dl, n, h, wd).transpose(1, 0, 2, 3)
    return np.ascontiguousarray(acc)


def partial_sums(vol, w, dtype=np.float64):
    """P (n, dl, 27, h, w) = sum_c w[c][tap] vol[c]: what the last aggregation layer's HEADP epilogue hands to k_softargmin_p"""
    return np.einsum("ct,ndchw->ndthw", np.asarray(w, dtype).reshape(32, 27), np.asarray(vol, dtype)).astype(dtype)


def shift_sum(P, bias, dtype=np.float64, order=0):
    """cost (n, dl, h, w) = bias + the 27 shifted values of P (n, dl, 27, h, w), zero outside the volume"""
    p = _pad3(np.asarray(P, dtype))
    n, dl, _, h, w = np.asarray(P).shape
    acc = np.full((n, dl, h, w), dtype(bias), dtype)
    taps = range(27) if order == 0 else reversed(range(27))
    for t in taps:
        dz, ky, kx = t // 9, (t // 3) % 3, t % 3
        acc = acc + p[:, dz:dz + dl, t, ky:ky + h, kx:kx + w]
    return acc


# ---- soft-argmin -----------------------------------------------------------------------------------------------------------
def soft_argmin(cost, dtype=np.float64, mut=None):
    """cost (n, dl, h, w) -> the expectation of d under softmax(-cost), (n, h, w)"""
    c = np.asarray(cost, dtype)
    if mut == "extra_zero_plane":
        c = np.concatenate([c, np.zeros_like(c[:, :1])], 1)
    d = np.arange(c.shape[1], dtype=dtype)[None, :, None, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        m = np.zeros_like(c[:, :1]) if mut == "no_max_subtraction" else (-c).max(1, keepdims=True)
        e = np.exp(-c - m)
        return ((d * e).sum(1) / e.sum(1)).astype(dtype)


def soft_argmin_bound(dl):
    """planes: the weights sum to one; each carries one rounded subtraction, one expf and at most dl additions (dl + 2 units of
    2^-24 relative), the quotient one more, times the largest plane index dl - 1; a factor of two is slack."""
    return (dl - 1) * (dl + 4) * 2.0 ** -23


SAM_REGIMES = ("spread1", "spread30", "above40", "below40")


def sam_inputs(n, dl, hl, wl, regime, seed):
    """Exact inputs of the soft-argmin hooks: volume (n, dl, 32, hl, wl) of small integers, weights (32, 27) multiples of 2^-4,
    bias a multiple of 2^-2 -> every partial sum of the contraction is a multiple of 2^-4 below 2^12: exact in fp32 in any order.
    Channel 0 has the centre tap alone (weight 1): its plane is added to the cost as it is, which carries the regime's spread and
    the planted pixels (the other channels are zeroed around a planted pixel, so its costs are exactly the planted ones):
    a one-hot minimum at d = 0, at dl - 1 and at an interior plane, two equal minima, and — shifted regimes — a pixel whose costs
    all lie near +-100, where exp() without the max-subtraction leaves the range of fp32.
    -> dict vol, w, bias, P (the partial sums of the same volume, exact), plants [(image, y, x, kind)]"""
    rng = np.random.default_rng(seed)
    w = rng.integers(-4, 5, (32, 27)).astype(np.float64) / 16.0
    w[0] = 0.0
    w[0, 13] = 1.0
    vol = (rng.integers(-1, 2, (n, dl, 32, hl, wl)) * (rng.random((n, dl, 32, hl, wl)) < 0.2)).astype(np.float64)
    shift = {"spread1": 0.0, "spread30": 0.0, "above40": 40.0, "below40": -40.0}[regime]
    if regime == "spread1":
        base = np.zeros((n, dl, hl, wl))
    elif regime == "spread30":
        base = rng.integers(-15, 16, (n, dl, hl, wl)).astype(np.float64)
    else:
        base = np.sign(shift) * (rng.integers(0, 31, (n, dl, hl, wl)).astype(np.float64) + 10.0)    # the other channels' noise (sigma 2) stays inside the 10
    vol[:, :, 0] = base
    kinds = ["min_first", "min_last", "min_inner", "two_minima"] + (["far"] if shift else [])
    pix = rng.permutation(n * hl * wl)[: len(kinds)]
    plants = []
    for k, g in zip(kinds, pix):
        i, y, x = g // (hl * wl), (g % (hl * wl)) // wl, g % wl
        plants.append((int(i), int(y), int(x), k))
        vol[i, :, 1:, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = 0.0
    for i, y, x, k in plants:
        mid = np.sign(shift) * 22.0             # planted costs: mid + 12, the minima at mid - 12 (shifted regimes: still beyond +-40)
        c = np.full(dl, mid + 12.0)
        if k == "min_first":
            c[0] = mid - 12.0
        elif k == "min_last":
            c[dl - 1] = mid - 12.0
        elif k == "min_inner":
            c[dl // 2] = mid - 12.0
        elif k == "two_minima":
            c[0] = c[dl - 1] = mid - 12.0
        else:
            c = np.sign(shift) * (60.0 + rng.integers(-5, 6, dl).astype(np.float64))              # +-(55 .. 65) on top of the bias
        vol[i, :, 0, y, x] = c
    bias = shift + 0.25
    return {"vol": vol.astype(np.float32), "w": w.astype(np.float32), "bias": np.float32(bias),
            "P": partial_sums(vol, w).astype(np.float32), "plants": plants}


# ---- refinement head ---------------------------------------------------------------------------------------------------------
def upsample(low, factor, h, w, dtype=np.float64, mut=None):
    """low (n, sh, sw) -> (n, h, w): bilinear, half-pixel centres, edge clamp, values x factor (upsample_map)"""
    a = np.asarray(low, dtype)
    n, sh, sw = a.shape

    def taps(n_out, n_low):
        i = np.arange(n_out, dtype=dtype)
        if mut == "align_corners":
            s = i * dtype((n_low - 1) / max(n_low * factor - 1, 1))
        else:
            s = (i + dtype(0.5)) * dtype(1.0 / factor) - dtype(0.5)
        if mut != "no_edge_clamp":
            s = np.maximum(s, dtype(0))
        i0 = np.floor(s).astype(np.int64)
        i1 = i0 + 1
        if mut != "no_edge_clamp":
            i1 = np.minimum(i1, n_low - 1)
        return i0, i1, (s - i0).astype(dtype)

    y0, y1, ly = taps(h, sh)
    x0, x1, lx = taps(w, sw)
    p = np.zeros((n, sh + 2, sw + 2), dtype)       # (only the mutant reaches the zero frame)
    p[:, 1:-1, 1:-1] = a
    g = lambda yi, xi: p[:, yi + 1][:, :, xi + 1]
    hy, hx = (1 - ly)[None, :, None], (1 - lx)[None, None, :]
    ly, lx = ly[None, :, None], lx[None, None, :]
    v = hy * (hx * g(y0, x0) + lx * g(y0, x1)) + ly * (hx * g(y1, x0) + lx * g(y1, x1))
    return (v * dtype(factor)).astype(dtype)


INV_Q = np.float32(1.0 / (192.0 * float(np.float32(spec.OUT_SCALE))))


def head(x, w, b, low, ups, dnorm, h_out, w_out, dtype=np.float64, order=0, mut=None):
    """x (n, 32, hk, wk), w (32, 9), low (n, hk / ups, wk / ups) -> dict disp (n, h_out, w_out), raw int32, mean_abs_dr.
    The 3x3 conv is zero-padded at the tensor edge hk x wk: a crop h_out < hk still reads the row below it."""
    xa = np.asarray(x, dtype)
    n, _, hk, wk = xa.shape
    if mut == "crop_edge_pad":
        xa = xa.copy()
        xa[:, :, h_out:] = 0
        xa[:, :, :, w_out:] = 0
    p = np.pad(xa, ((0, 0), (0, 0), (1, 1), (1, 1)))
    wt = np.asarray(w, dtype).reshape(32, 9)
    acc = np.full((n, hk, wk), dtype(b), dtype)
    pairs = [(c, t) for c in range(32) for t in range(9)]
    if order == 1:
        pairs = [(c, t) for t in reversed(range(9)) for c in reversed(range(32))]
    for c, t in pairs:
        if wt[c, t] != 0:
            acc = acc + wt[c, t] * p[:, c, t // 3:t // 3 + hk, t % 3:t % 3 + wk]
    acc = acc[:, :h_out, :w_out]
    up = upsample(low, ups, h_out, w_out, dtype, mut=mut if mut in ("no_edge_clamp", "align_corners") else None)
    moved = dtype(dnorm) * acc
    d = (up + moved).astype(dtype)
    disp = np.where(d > 0, d, dtype(0)).astype(dtype)
    if mut == "col62_from_61" and w_out > 62:
        disp = disp.copy()
        disp[:, :, 62] = disp[:, :, 61]
    raw = np.rint(disp.astype(np.float32) * INV_Q).astype(np.int32)
    return {"disp": disp, "raw": raw, "mean_abs_dr": float(np.abs(np.asarray(moved, np.float64)).mean())}


def head_exact_inputs(n, hk, wk, ups, seed):
    """x = i + j 2^-12 with small integers i (|i| <= 2, sparse) and j in {-1, 0, 1}: the fp16 hi part is i (or x itself where i = 0)
    and the lo part j 2^-12, 22 significant bits at most; weights k 2^-6 (|k| <= 4: exact in fp16, so their lo part is zero), bias
    a multiple of 2^-6, dnorm 64, low = 0.  |acc| <= 288 * 2 / 16 + 1 < 2^6 and every partial sum is a multiple of 2^-18: 24 bits."""
    rng = np.random.default_rng(seed)
    i = rng.integers(-2, 3, (n, 32, hk, wk)) * (rng.random((n, 32, hk, wk)) < 0.35)
    j = rng.integers(-1, 2, (n, 32, hk, wk))
    x = (i + j * 2.0 ** -12).astype(np.float32)
    w = (rng.integers(-4, 5, (32, 9)) / 64.0).astype(np.float32)
    b = np.float32(rng.integers(-8, 9) / 64.0)
    low = np.zeros((n, hk // ups, wk // ups), np.float32)
    return x, w, b, low


# ---- image pyramid -----------------------------------------------------------------------------------------------------------
def pyramid(in6, levels, dtype=np.float64):
    """in6 int8 (n, 6, h, w) -> [level 1 .. levels - 1], level k (n, 3, hp >> k, wp >> k): the left eye / 128, zero-padded to
    hp x wp = ceil16, pooled 2x2 once per level"""
    a = np.asarray(in6)
    n, _, h, w = a.shape
    hp, wp = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    cur = np.zeros((n, 3, hp, wp), dtype)
    cur[:, :, :h, :w] = a[:, :3].astype(dtype) / dtype(128)
    out = []
    for _ in range(1, levels):
        cur = ((cur[:, :, 0::2, 0::2] + cur[:, :, 0::2, 1::2]) + (cur[:, :, 1::2, 0::2] + cur[:, :, 1::2, 1::2])) * dtype(0.25)
        out.append(cur.astype(dtype))
    return out


# ---- the shapes of tests/test_gpu_midstage.py (shared with the CPU test of the references) ----------------------------------
# (n, dl, hl, wl): 63 pixels in one workgroup across two image boundaries; 130 pixels, a workgroup that straddles the two images
# and one with 2 live lanes; dl = 1, 2, 15, 16 (the guards of the unrolled loops); one row, one column, one pixel (wl < dl)
SAM_SHAPES = [(1, 1, 3, 5), (3, 2, 3, 7), (2, 3, 5, 13), (1, 12, 6, 10), (2, 15, 4, 9), (2, 16, 1, 40), (1, 16, 8, 1), (1, 16, 1, 1)]
# the 8 x 16 tiles of the aggregation kernels on both axes; n = 2: the zero plane two pairs share in the padded layout
TAIL_SHAPES = [(1, 1, 8, 16), (2, 3, 4, 6), (1, 6, 17, 33), (2, 16, 9, 17)]
# (hk, wk, h_out, w_out, ups, n): one tile; one column short of the 62-column tile; ONE column in the second tile; crops on both
# axes; a x2 level with three images; a x2 level of one tile
HEAD_SHAPES = [(16, 16, 16, 16, 16, 1), (16, 64, 16, 61, 16, 1), (16, 64, 15, 63, 16, 1), (32, 80, 31, 67, 16, 2),
               (48, 128, 48, 125, 2, 3), (32, 32, 32, 32, 2, 1)]
PYR_SHAPES = [(2, 38, 124), (1, 17, 33), (1, 64, 96)]        # (n, h, w) at levels = 4
UPS_SHAPES = HEAD_SHAPES + [(64, 16, 64, 16, 16, 1)]          # + an N x 1 low map (the 16-row shapes have 1 x N ones)


# ---- the criteria of tests/test_gpu_midstage.py, as predicates (the CPU test applies them to the mutants) --------------------
def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(bits(a), bits(b)))


def sam_disp_error(disp, cost):
    """max |disp - float64 soft-argmin of the given costs| in planes (inf when a value is not finite)"""
    d = np.asarray(disp, np.float64)
    if not np.isfinite(d).all():
        return float("inf")
    return float(np.abs(d - soft_argmin(np.asarray(cost, np.float64))).max())


def upsample_lows(n, sh, sw, seed):
    """a disparity-like low map with zeros (the relu has nothing to clip: values >= 0) and values up to 11"""
    rng = np.random.default_rng(seed)
    low = (rng.random((n, sh, sw)) * 11.0).astype(np.float32)
    low[rng.random((n, sh, sw)) < 0.2] = 0.0
    low[:, 0, 0] = 7.5                   # the corner every clamp touches is never zero
    low[:, -1, -1] = 9.25
    return low


def upsample_bound(low, factor):
    """six roundings in upsample_map's expression (two inner sums of two products, the outer sum, the factor)"""
    return 6.0 * 2.0 ** -24 * float(np.abs(low).max()) * factor
