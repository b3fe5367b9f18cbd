"""References for the persistent kernels of the towers and the low-resolution convolutions (tests/test_tower_refs.py proves them
on the CPU, tests/test_gpu_tower_grids.py holds the sn_dbg_* hooks to them at every grid size): one 3x3 tower layer, one
residual block, the tail (block + head + upsample + wire map), the 5x5 stride-2 and 3x3x3 layers of the low-resolution branch,
the first down-conv(s) and the refinement input conv.  Everything is numpy float64 unless a dtype says otherwise.

Two input families.
EXACT: small integers and multiples of small powers of two, chosen so that every partial sum of every accumulator is a multiple
of one grid 2^g and smaller than 2^(g + 24): exact in fp32 in ANY order.  `budget` proves that from the operands (the sum of the
absolute terms bounds every partial sum of every order), so the result is one bit pattern whatever the MFMA order, the tile
shape or the schedule, and the float64 reference IS that pattern.
RANDOM: standard-normal operands, as the existing per-kernel tests use.

Arithmetic of the kernels, as the references model it:
  fp16 tower (SN_PREC_F16)      operands fp16, sums fp32, a stored value is h = fp16(v); out = max(h, fp16(h * fp16(0.2)))
                                (act_pack2_f16: round first, then LeakyReLU on the fp16 value)
  split operands (F16X3, x3s)   a value is hi + lo / 2048 with hi = fp16(v), lo = fp16((v - hi) 2048); a product x w is
                                xh wh + (xh wl + xl wh) / 2048 (the xl wl term is dropped); v = acc0 + acc1 / 2048 + bias
                                (+ residual), LeakyReLU max(v, v * 0.2f) in fp32, then the value is stored as a pair again
"""
from __future__ import annotations

import numpy as np

import midstage_ref as mr

F16, F32, F64 = np.float16, np.float32, np.float64
SLOPE16 = F64(F16(0.2))          # the fp16 tower's slope: 0.199951171875
SLOPE32 = F32(0.2)


# ---- number formats ----------------------------------------------------------------------------------------------------------
def q16(a):
    """round to fp16, returned in the dtype of a (float64 / float32: one rounding either way)"""
    a = np.asarray(a)
    return a.astype(F16).astype(a.dtype)


def act16(v, lrelu=True):
    """the fp16 tower's store: h = fp16(v), then max(h, fp16(h * fp16(0.2))) — the product is exact in float64, so one rounding"""
    h = q16(np.asarray(v, F64))
    return np.maximum(h, q16(h * SLOPE16)) if lrelu else h


def split(v):
    """float32 value -> (hi, lo') float32: hi = fp16(v), lo' = fp16((v - hi) 2048)"""
    v = np.asarray(v, F32)
    hi = v.astype(F16).astype(F32)
    return hi, ((v - hi) * F32(2048)).astype(F16).astype(F32)


def join(hi, lo):
    return (np.asarray(hi, F32) + np.asarray(lo, F32) * F32(1.0 / 2048.0)).astype(F32)


def store_x3(v, lrelu=True):
    """epilogue of the split-operand kernels on the fp32 value v: LeakyReLU in fp32, then the hi / lo pair, read back in fp32"""
    v = np.asarray(v, F32)
    if lrelu:
        v = np.maximum(v, v * SLOPE32)
    return join(*split(v))


def lrelu64(v):
    return np.where(v > 0, v, v * F64(SLOPE32))


# ---- convolutions --------------------------------------------------------------------------------------------------------
def conv(x, w, b=None, dil=1, stride=1, dtype=F64):
    """x (n, ci, h, w), w (co, ci, k, k), zero padding (k // 2) dil -> (n, co, ho, wo); one BLAS product per tap"""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    n, ci, h, wd = x.shape
    co, _, k, _ = w.shape
    pad = (k // 2) * dil
    ho, wo = (h + stride - 1) // stride, (wd + stride - 1) // stride
    p = np.pad(x, ((0, 0), (0, 0), (pad, pad + stride), (pad, pad + stride)))
    acc = np.zeros((n, co, ho, wo), dtype)
    for ky in range(k):
        for kx in range(k):
            patch = p[:, :, ky * dil: ky * dil + ho * stride: stride, kx * dil: kx * dil + wo * stride: stride]
            acc += np.einsum("oc,nchw->nohw", w[:, :, ky, kx], patch, optimize=True)
    if b is not None:
        acc += np.asarray(b, dtype)[None, :, None, None]
    return acc


def conv_ordered(x, w, b, dil=1, stride=1, dtype=F32, order=0):
    """the same convolution as an explicit sequence of additions in `dtype`: bias first, then the (ci, tap) terms forwards
    (order 0) or backwards (order 1).  Slow: for the CPU test's proof that the exact inputs do not care about the order."""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    n, ci, h, wd = x.shape
    co, _, k, _ = w.shape
    pad = (k // 2) * dil
    ho, wo = (h + stride - 1) // stride, (wd + stride - 1) // stride
    p = np.pad(x, ((0, 0), (0, 0), (pad, pad + stride), (pad, pad + stride)))
    acc = np.zeros((n, co, ho, wo), dtype) + np.asarray(b, dtype)[None, :, None, None]
    terms = [(c, ky, kx) for c in range(ci) for ky in range(k) for kx in range(k)]
    for c, ky, kx in (terms if order == 0 else reversed(terms)):
        patch = p[:, c, ky * dil: ky * dil + ho * stride: stride, kx * dil: kx * dil + wo * stride: stride]
        acc = (acc + w[None, :, c, ky, kx, None, None] * patch[:, None]).astype(dtype)
    return acc


def conv3d(x, w, b=None, dtype=F64):
    """x (ci, d, h, w), w (co, ci, 3, 3, 3), zero padding 1 -> (co, d, h, w)"""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    ci, d, h, wd = x.shape
    p = np.pad(x, ((0, 0), (1, 1), (1, 1), (1, 1)))
    acc = np.zeros((w.shape[0], d, h, wd), dtype)
    for dz in range(3):
        for ky in range(3):
            for kx in range(3):
                acc += np.einsum("oc,cdhw->odhw", w[:, :, dz, ky, kx], p[:, dz:dz + d, ky:ky + h, kx:kx + wd], optimize=True)
    if b is not None:
        acc += np.asarray(b, dtype)[:, None, None, None]
    return acc


# ---- the operations, float64 -------------------------------------------------------------------------------------------------
def layer_f16(x, w, b, dil=1, res=None, lrelu=True):
    """one layer of the fp16 tower (k_ref_conv_f16_v2) on fp16-representable operands"""
    v = conv(x, w, b, dil)
    return act16(v if res is None else v + np.asarray(res, F64), lrelu)


def block_f16(x, w1, b1, w2, b2, dil=1):
    """y = act16(x + conv2(act16(conv1(x) + b1)) + b2): the residual block of the fp16 tower, streamed or as two launches"""
    t = act16(conv(x, w1, b1, dil))
    return act16(np.asarray(x, F64) + conv(t, w2, b2, dil))


def tail_f16(x, w1, b1, w2, b2, head_w, head_b, low, ups, dnorm, h_out, w_out):
    """the last block followed by the refinement head (3x3 32 -> 1 on the fp16 y, relu(upsample(low) + dnorm r), wire rounding)"""
    y = block_f16(x, w1, b1, w2, b2, 1)
    out = mr.head(y, head_w, head_b, low, ups, dnorm, h_out, w_out, F64)
    r = conv(y, np.asarray(head_w, F64).reshape(1, 32, 3, 3), [head_b])[:, 0, :h_out, :w_out]
    out["pre"] = mr.upsample(low, ups, h_out, w_out) + F64(dnorm) * r        # disp = relu(pre): the conditions look at this
    return out


def _bias(b, caxis, ndim):
    shape = [1] * ndim
    shape[caxis] = -1
    return np.asarray(b, F64).reshape(shape)


def sums_x3(x, w, b, conv_fn, res=None, caxis=1):
    """the split-operand sum in float64: acc0 + acc1 / 2048 + bias (+ residual pair) -> v"""
    xh, xl = split(x)
    wh, wl = split(w)
    acc0 = conv_fn(xh, wh)
    acc1 = conv_fn(xh, wl) + conv_fn(xl, wh)
    v = acc0 + acc1 / 2048.0 + _bias(b, caxis, acc0.ndim)
    if res is not None:
        v = v + join(*split(res)).astype(F64)
    return v


def layer_x3(x, w, b, dil=1, stride=1, res=None, lrelu=True):
    """one split-operand layer (k_ref_conv_f16x3, k_conv_x3s, k_feat_x3s_dma, k_down_x3s_dma) as the kernel evaluates it.
    The float32 cast is exact for the exact family (budget); for random operands it is the kernel's own rounding."""
    v = sums_x3(x, w, b, lambda a, k: conv(a, k, None, dil, stride), res)
    return store_x3(v.astype(F32), lrelu)


def layer3d_x3(x, w, b, lrelu=True):
    """k_agg_x3s_dma / the 96-channel k_conv_x3s on a volume x (32, d, h, w)"""
    v = sums_x3(x, w, b, lambda a, k: conv3d(a, k), caxis=0)
    return store_x3(v.astype(F32), lrelu)


def block_x3(x, w1, b1, w2, b2, dil=1):
    t = layer_x3(x, w1, b1, dil)
    return layer_x3(t, w2, b2, dil, res=x)


def layer_f32(x, w, b, dil=1, res=None, lrelu=True):
    """the fp32 tower layer (k_ref_conv_f32): plain fp32 operands, LeakyReLU max(v, v * 0.2f)"""
    v = conv(x, w, b, dil)
    if res is not None:
        v = v + np.asarray(res, F64)
    v = v.astype(F32)
    return np.maximum(v, v * SLOPE32) if lrelu else v


def truth_layer(x, w, b, dil=1, stride=1, res=None, lrelu=True):
    """plain float64 mathematics of a layer on the operands as given (what the random family is judged against)"""
    v = conv(x, w, b, dil, stride)
    if res is not None:
        v = v + np.asarray(res, F64)
    return lrelu64(v) if lrelu else v


def truth_block(x, w1, b1, w2, b2, dil=1, round_t=None):
    """round_t = q16: the fp16 tower holds t in fp16 (the existing fp16 test's reference does the same)"""
    t = truth_layer(x, w1, b1, dil)
    return truth_layer(t if round_t is None else round_t(t), w2, b2, dil, res=x)


def down0(in6, w, b, dtype=F64):
    """in6 int8 (6, h, w) -> (2, 32, hp / 2, wp / 2): both eyes / 128, zero-padded to hp x wp = ceil16, 5x5 stride 2, no activation"""
    a = np.asarray(in6)
    _, h, wd = a.shape
    hp, wp = (h + 15) // 16 * 16, (wd + 15) // 16 * 16
    x = np.zeros((2, 3, hp, wp), dtype)
    x[:, :, :h, :wd] = a.reshape(2, 3, h, wd).astype(dtype) / dtype(128)
    return conv(x, w, b, 1, 2, dtype)


def down01(in6, w0, b0, w1, b1):
    """the first two down-convs (the folded 13x13 stride-4 kernel computes exactly this, zero padding of the half-resolution
    map included)"""
    return conv(down0(in6, w0, b0), w1, b1, 1, 2)


def refin_input(disp_low, in6, dmax):
    """the four input planes of ref.in: upsample16(disp_low) / dmax, then Y, U, V of the left eye / 128 — (n, 4, hp, wp)"""
    a = np.asarray(in6)
    n, _, h, wd = a.shape
    hp, wp = (h + 15) // 16 * 16, (wd + 15) // 16 * 16
    x = np.zeros((n, 4, hp, wp), F64)
    x[:, 0] = mr.upsample(disp_low, 16, hp, wp) / F64(dmax)
    x[:, 1:, :h, :wd] = a[:, :3].astype(F64) / 128.0
    return x


# ---- the exactness proof -----------------------------------------------------------------------------------------------------
def grid_exp(*arrays):
    """largest g such that every element of every array is a multiple of 2^g (arrays of all zeros do not count)"""
    g = None
    for a in arrays:
        a = np.asarray(a, F64).ravel()
        a = a[a != 0]
        if a.size == 0:
            continue
        m, e = np.frexp(a)
        mi = np.abs(m * 2.0 ** 53).astype(np.int64)
        tz = np.log2((mi & -mi).astype(F64)).astype(np.int64)
        ga = int((e - 53 + tz).min())
        g = ga if g is None else min(g, ga)
    return 0 if g is None else g


def budget(abs_sum_max, g):
    """bits a partial sum can need: every partial sum, in any order, is a multiple of 2^g below abs_sum_max.  <= 24: exact in fp32"""
    return 0.0 if abs_sum_max == 0 else float(np.log2(abs_sum_max)) - g


def budget_conv(x, w, b=None, res=None, conv_fn=None, caxis=1, **kw):
    """budget of bias + sum x w (+ residual) from the operands alone"""
    fn = conv_fn or (lambda a, k: conv(a, k, None, **kw))
    tot = fn(np.abs(np.asarray(x, F64)), np.abs(np.asarray(w, F64)))
    g = grid_exp(x) + grid_exp(w)
    if b is not None:
        tot, g = tot + np.abs(_bias(b, caxis, tot.ndim)), min(g, grid_exp(b))
    if res is not None:
        tot, g = tot + np.abs(np.asarray(res, F64)), min(g, grid_exp(res))
    return budget(float(tot.max()), g)


def budget_refin(x4, w, b):
    """ref.in: the disparity plane (hi / lo pair, weights without a lo part) and the image planes (no lo part, split weights) have
    grids of their own; the sum lives on the finer one"""
    tot = conv(np.abs(x4), np.abs(np.asarray(w, F64))) + np.abs(_bias(b, 1, 4))
    g = min(grid_exp(x4[:, :1]) + grid_exp(w[:, :1]), grid_exp(x4[:, 1:]) + grid_exp(w[:, 1:]), grid_exp(b))
    return budget(float(tot.max()), g)


def budget_x3(x, w, b, res=None, conv_fn=None, caxis=1, **kw):
    """the split-operand layer: acc0 = sum xh wh, acc1 = sum (xh wl + xl wh), and v = acc0 + acc1 / 2048 + bias (+ residual hi +
    lo / 2048) with every addend on one grid.  -> the largest of the three budgets"""
    fn = conv_fn or (lambda a, k: conv(a, k, None, **kw))
    xh, xl = split(x)
    wh, wl = split(w)
    ab = lambda a: np.abs(np.asarray(a, F64))
    a0 = fn(ab(xh), ab(wh))
    a1 = fn(ab(xh), ab(wl)) + fn(ab(xl), ab(wh))
    g0 = grid_exp(xh) + grid_exp(wh)
    g1 = min(grid_exp(xh) + grid_exp(wl), grid_exp(xl) + grid_exp(wh))
    tot = a0 + a1 / 2048.0 + np.abs(_bias(b, caxis, a0.ndim))
    gv = min(g0, g1 - 11, grid_exp(b))
    if res is not None:
        rh, rl = split(res)
        tot = tot + ab(rh) + ab(rl) / 2048.0
        gv = min(gv, grid_exp(rh), grid_exp(rl) - 11)
    return max(budget(float(a0.max()), g0), budget(float(a1.max()), g1), budget(float(tot.max()), gv))


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def exact_f16_layer(n, h, w, seed, res=False):
    """x in {-2..2}, weights in {-2..2} / 8, a zero-centred bias (2 k + 1) / 16 (so the LeakyReLU's negative branch is taken
    about half the time, and no sum is exactly zero), residual in {-2..2}: every sum a multiple of 1/16 below 2^8"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, (n, 32, h, w)).astype(F32)
    wt = (rng.integers(-2, 3, (32, 32, 3, 3)) / 8.0).astype(F32)
    b = ((2 * rng.integers(-16, 16, 32) + 1) / 16.0).astype(F32)
    r = rng.integers(-2, 3, (n, 32, h, w)).astype(F32) if res else None
    return x, wt, b, r


def exact_f16_block(n, h, w, seed):
    """x in {-2..2}, weights in {-2..2} / 8, b1 = 160 + k / 8: conv1's output stays positive (|sum| <= 288 * 2 * 2 / 8 = 144), so
    t = fp16(v) is a multiple of 1/8 and conv2's inputs stay on a fixed grid; b2 = k / 8 zero-centred, so about half of the
    block's outputs take the negative branch"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, (n, 32, h, w)).astype(F32)
    w1 = (rng.integers(-2, 3, (32, 32, 3, 3)) / 8.0).astype(F32)
    w2 = (rng.integers(-2, 3, (32, 32, 3, 3)) / 8.0).astype(F32)
    b1 = (160.0 + rng.integers(-16, 17, 32) / 8.0).astype(F32)
    b2 = (rng.integers(-16, 17, 32) / 8.0).astype(F32)
    return x, w1, b1, w2, b2


def _sparse(rng, shape, per_out, lo, hi):
    """integer weights (co, ...) with exactly per_out non-zero entries per output channel, each in [lo, hi] \\ {0}"""
    co = shape[0]
    m = int(np.prod(shape[1:]))
    w = np.zeros((co, m), F64)
    vals = np.array([v for v in range(lo, hi + 1) if v != 0], F64)
    for o in range(co):
        idx = rng.choice(m, per_out, replace=False)
        w[o, idx] = rng.choice(vals, per_out)
    return w.reshape(shape)


def exact_f16_tail(n, hk, wk, ups, seed):
    """The tail's head needs y on a fixed grid too, so BOTH convs stay positive here (the negative branch of the block's output is
    the block cases' job): 36 non-zero weights in {+-1, +-2} / 8 per output channel, b1 = 20 + k / 8 (|conv1| <= 36 * 2 * 2 / 8 =
    18: t in (2, 38), multiples of 1/8), b2 = 352 + k / 8 (|conv2| <= 36 * 38 / 4 = 342: y in (8, 700), multiples of 2^-6).
    Head: 32 non-zero weights k / 64 (|k| <= 4, exact in fp16: no lo part) and a bias (an odd multiple of 2^-11) that centres r on
    its median, dnorm 64, low = 0: |r| < 2^11 on a grid of 2^-12, disp = relu(64 r) clips about half the pixels."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, (n, 32, hk, wk)).astype(F32)
    w1 = (_sparse(rng, (32, 32, 3, 3), 36, -2, 2) / 8.0).astype(F32)
    w2 = (_sparse(rng, (32, 32, 3, 3), 36, -2, 2) / 8.0).astype(F32)
    b1 = (20.0 + rng.integers(-8, 9, 32) / 8.0).astype(F32)
    b2 = (352.0 + rng.integers(-8, 9, 32) / 8.0).astype(F32)
    hw = (_sparse(rng, (1, 32, 9), 32, -4, 4)[0] / 64.0).astype(F32)
    r0 = conv(block_f16(x, w1, b1, w2, b2, 1), hw.reshape(1, 32, 3, 3))
    hb = F32(-(np.round(float(np.median(r0)) * 64.0) / 64.0 + 2.0 ** -11))      # off r0's grid (2^-8 .. 2^-10): r is never exactly zero
    low = np.zeros((n, hk // ups, wk // ups), F32)
    return x, w1, b1, w2, b2, hw, hb, low


def exact_x3_layer(n, ci, h, w, seed, k=3, res=False, xmax=2):
    """Split operands with lo parts in BOTH: x = i + j 2^-12 (hi = i, lo' = j / 2; j = 0 where i = 0, so that no hi part is tiny),
    w = k / 8 + m 2^-15 (hi = k / 8, lo' = m / 16; m = 0 where k = 0: 2^-15 alone is an fp16 subnormal), bias k / 8, residual like x.
    acc0 is a multiple of 1/8, acc1 of 1/16, v of 2^-15 below 2^8 (budget_x3 checks the actual operands)."""
    rng = np.random.default_rng(seed)
    i = rng.integers(-xmax, xmax + 1, (n, ci, h, w))
    j = rng.integers(-1, 2, (n, ci, h, w)) * (i != 0)
    x = (i + j * 2.0 ** -12).astype(F32)
    kk = rng.integers(-2, 3, (32, ci, k, k))
    m = rng.integers(-1, 2, (32, ci, k, k)) * (kk != 0)
    wt = (kk / 8.0 + m * 2.0 ** -15).astype(F32)
    b = (rng.integers(-16, 17, 32) / 8.0).astype(F32)
    r = None
    if res:
        ri = rng.integers(-2, 3, (n, 32, h, w))
        r = (ri + rng.integers(-1, 2, (n, 32, h, w)) * (ri != 0) * 2.0 ** -12).astype(F32)
    return x, wt, b, r


def exact_x3_block(n, h, w, seed):
    """The split block keeps 22 bits of t, so conv2's sums stay on one grid only if they are short: x = i + j 2^-12 as
    exact_x3_layer; w1: 36 non-zero weights k / 8 + m 2^-15 per output channel, b1 = 20 + k / 8, so that t = v1 lies in (2, 38) on a
    grid of 2^-15 (20.3 bits: the hi / lo pair holds it exactly, and its lo part is not zero); w2: FOUR non-zero weights +-1/8 per
    output channel and no lo part (t_hi * wl / 2048 would be a multiple of 2^-24), b2 = (2 k + 1) / 16 zero-centred: v2 is a multiple
    of 2^-18 below 2^5.  conv2's weight lo path and its other taps are the random family's job."""
    rng = np.random.default_rng(seed)
    i = rng.integers(-2, 3, (n, 32, h, w))
    x = (i + rng.integers(-1, 2, i.shape) * (i != 0) * 2.0 ** -12).astype(F32)
    kk = _sparse(rng, (32, 32, 3, 3), 36, -2, 2)
    w1 = (kk / 8.0 + rng.integers(-1, 2, kk.shape) * (kk != 0) * 2.0 ** -15).astype(F32)
    w2 = (_sparse(rng, (32, 32, 3, 3), 4, -1, 1) / 8.0).astype(F32)
    b1 = (20.0 + rng.integers(-8, 9, 32) / 8.0).astype(F32)
    b2 = ((2 * rng.integers(-16, 16, 32) + 1) / 16.0).astype(F32)
    return x, w1, b1, w2, b2


def exact_int8(n, h, w, seed):
    """int8 model input, multiples of 8 (x / 128 is a multiple of 2^-4): room for the lo parts of the weights"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-16, 16, (n, 6, h, w)) * 8).astype(np.int8)


def exact_x3_volume(d, h, w, seed):
    """the 3x3x3 aggregation layer (864 terms): x = i + j 2^-12 with i in {-1, 0, 1}, weights and bias as exact_x3_layer"""
    rng = np.random.default_rng(seed)
    i = rng.integers(-1, 2, (32, d, h, w))
    x = (i + rng.integers(-1, 2, (32, d, h, w)) * (i != 0) * 2.0 ** -12).astype(F32)
    kk = rng.integers(-2, 3, (32, 32, 3, 3, 3))
    wt = (kk / 8.0 + rng.integers(-1, 2, kk.shape) * (kk != 0) * 2.0 ** -15).astype(F32)
    return x, wt, (rng.integers(-16, 17, 32) / 8.0).astype(F32)


def exact_down0(n, h, w, seed):
    """in6 multiples of 8, weights k / 8 + m 2^-15 (|k| <= 2), bias k / 8: 75 terms on a grid of 2^-19"""
    rng = np.random.default_rng(seed)
    kk = rng.integers(-2, 3, (32, 3, 5, 5))
    wt = (kk / 8.0 + rng.integers(-1, 2, kk.shape) * (kk != 0) * 2.0 ** -15).astype(F32)
    return exact_int8(n, h, w, seed + 1), wt, (rng.integers(-16, 17, 32) / 8.0).astype(F32)


def exact_down01(n, h, w, seed):
    """Both down-convs with weights in {-1, 0, 1} / 8 and NO lo parts: the folded 13x13 weights are then multiples of 1/64 below
    8 (exact in fp16) and every sum a multiple of 2^-10.  With lo parts the folded weights need their 22 bits and the 507-term
    sums leave the fp32 grid: the lo path of this kernel is the random family's job."""
    rng = np.random.default_rng(seed)
    w0 = (rng.integers(-1, 2, (32, 3, 5, 5)) / 8.0).astype(F32)
    w1 = (rng.integers(-1, 2, (32, 32, 5, 5)) / 8.0).astype(F32)
    b0 = (rng.integers(-8, 9, 32) / 8.0).astype(F32)
    b1 = ((2 * rng.integers(-8, 8, 32) + 1) / 16.0).astype(F32)
    return exact_int8(n, h, w, seed + 1), w0, b0, w1, b1


def exact_refin(n, h, w, seed, dmax=64):
    """in6 multiples of 8; disp_low in {0..4}: the x16 bilinear weights are multiples of 1/32, so d = 16 up / dmax is a multiple of
    2^-12 in [0, 1] — fp16 holds 11 bits of it and the lo part the rest.  Image weights k / 8 + m 2^-15; the disparity plane's
    weights k / 8 without a lo part (d_hi * wl / 2048 would be a multiple of 2^-27), bias k / 8."""
    rng = np.random.default_rng(seed)
    hp, wp = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    kk = rng.integers(-2, 3, (32, 4, 3, 3))
    m = rng.integers(-1, 2, kk.shape) * (kk != 0)
    m[:, 0] = 0
    wt = (kk / 8.0 + m * 2.0 ** -15).astype(F32)
    dl = rng.integers(0, 5, (n, hp // 16, wp // 16)).astype(F32)
    return dl, exact_int8(n, h, w, seed + 1), dmax, wt, (rng.integers(-16, 17, 32) / 8.0).astype(F32)


def random_layer(n, h, w, seed, fp16=False, k=3, ci=32):
    """standard-normal x and residual, weights / 17 (5x5: / 28), as tests/test_gpu_f16.py; fp16: operands rounded to fp16"""
    rng = np.random.default_rng(seed)
    rnd = (lambda a: q16(a.astype(F32))) if fp16 else (lambda a: a.astype(F32))
    x = rnd(rng.standard_normal((n, ci, h, w)))
    wt = rnd(rng.standard_normal((32, ci, k, k)) / (17.0 if k == 3 else 28.0))
    b = rng.standard_normal(32).astype(F32)
    r = rnd(rng.standard_normal((n, 32, h, w)))
    return x, wt, b, r


def random_block(n, h, w, seed, fp16=False):
    rng = np.random.default_rng(seed)
    rnd = (lambda a: q16(a.astype(F32))) if fp16 else (lambda a: a.astype(F32))
    x = rnd(rng.standard_normal((n, 32, h, w)))
    w1 = rnd(rng.standard_normal((32, 32, 3, 3)) / 17.0)
    w2 = rnd(rng.standard_normal((32, 32, 3, 3)) / 17.0)
    return x, w1, rng.standard_normal(32).astype(F32), w2, rng.standard_normal(32).astype(F32)


# ---- conditions on a reference output ----------------------------------------------------------------------------------------
def conditions(ref, strip=None, lrelu=True):
    """-> dict: duplicate row pieces (per channel, over all images, rows — hence row phases — and strips of `strip` columns; a
    last strip narrower than 16 columns counts with the one before it: a handful of quantised values does repeat),
    share of zeros, share of negatives.  check_conditions asserts the limits."""
    a = np.asarray(ref)
    n, c, h, w = a.shape
    strip = strip or w
    starts = list(range(0, w, strip))
    if len(starts) > 1 and w - starts[-1] < 16:
        starts.pop()
    ends = starts[1:] + [w]
    dup = 0
    for ch in range(c):
        seen = set()
        for x0, x1 in zip(starts, ends):
            piece = np.ascontiguousarray(a[:, ch, :, x0:x1]).reshape(n * h, -1)
            for row in piece:
                key = (row.size, row.tobytes())
                dup += key in seen
                seen.add(key)
    return {"dup": dup, "zero": float((a == 0).mean()), "neg": float((a < 0).mean())}


def check_conditions(ref, strip=None, lrelu=True, what=""):
    c = conditions(ref, strip, lrelu)
    assert c["dup"] == 0, (what, c)
    assert c["zero"] < 1e-3, (what, c)
    if lrelu:
        assert 0.2 <= c["neg"] <= 0.8, (what, c)
    return c


# ---- the schedule of the streamed blocks (launch_ref_block_stream*, StreamIter) ---------------------------------------------
STREAM_OW_F16 = {1: 62, 2: 60, 4: 120, 8: 112}      # StreamTile1 / 2 / 4 / 8: TW - 2 DIL with TW = 64, 64, 128, 128
STREAM_OW_TAIL = 60                                  # StreamTileTail: one more column on every side for the head
STREAM_OW_X3 = {1: 62, 2: 60, 4: 56, 8: 48}         # StreamTileX3<DIL, 64, ...>::OW = 64 - 2 DIL


def stream_sched(n, h, w, dil, ow, cus):
    nstrips, hsub = (w + ow - 1) // ow, (h + dil - 1) // dil
    total = n * dil * nstrips * hsub
    nwg = max(1, min(cus, total))
    rpw = (total + nwg - 1) // nwg
    return {"nstrips": nstrips, "hsub": hsub, "total": total, "rpw": rpw, "grid": (total + rpw - 1) // rpw, "dil": dil, "n": n}


def stream_caps(total, max_cus):
    """the smallest cap for every distinct rows_per_wg a cap in 1 .. max_cus gives; the first is 1: the whole launch in one workgroup"""
    caps, seen = [], set()
    for c in range(1, min(max_cus, total) + 1):
        rpw = (total + c - 1) // c
        if rpw not in seen:
            seen.add(rpw)
            caps.append(c)
    return caps


def stream_shares(s):
    """-> per workgroup the list of its units (strip-phase sp, v0, v1), as StreamIter::next_unit cuts them"""
    out = []
    for f0 in range(0, s["total"], s["rpw"]):
        f1, f, units = min(f0 + s["rpw"], s["total"]), f0, []
        while f < f1:
            sp, v0 = divmod(f, s["hsub"])
            ln = min(s["hsub"] - v0, f1 - f)
            units.append((sp, v0, v0 + ln))
            f += ln
        out.append(units)
    return out


def stream_events(s):
    """what the shares of one schedule exercise: a share of >= 3 units, a share that starts mid-strip, a share that crosses an image
    boundary, a unit of length 1"""
    per_img = s["dil"] * s["nstrips"]
    ev = set()
    for units in stream_shares(s):
        if len(units) >= 3:
            ev.add("three_units")
        if units[0][1] > 0:
            ev.add("mid_strip")
        if len({sp // per_img for sp, _, _ in units}) > 1:
            ev.add("image_boundary")
        if any(v1 - v0 == 1 for _, v0, v1 in units):
            ev.add("unit_of_one")
    return ev


STREAM_EVENTS = {"three_units", "mid_strip", "image_boundary", "unit_of_one"}


# ---- mutations: what a broken schedule does to an output -------------------------------------------------------------------
MUTATIONS = ("row_unwritten", "first_row_from_above", "strips_swapped", "phases_swapped", "image_from_next", "tile_skipped",
             "channel_block_from_neighbour")


def mutate(ref, mut, dil=1, strip=62, tile=(8, 64)):
    """ref (n, 32, h, w) -> a copy with ONE defect of a persistent schedule, placed away from the tensor's edges"""
    a = np.array(ref, copy=True)
    n, _, h, w = a.shape
    y = min(h - 1, max(2 * dil, h // 2))
    th, tw = tile
    if mut == "row_unwritten":              # one output row of one unit: the strip's columns of one row keep the pre-fill
        a[n - 1, :, y, strip:min(2 * strip, w)] = np.nan
    elif mut == "first_row_from_above":     # a unit restarts one step early: its first row is the row above it in its phase
        a[0, :, y, :strip] = ref[0, :, y - dil, :strip]
    elif mut == "strips_swapped":           # strip index off by one
        k = min(strip, w - strip)
        a[0, :, y, :k], a[0, :, y, strip:strip + k] = ref[0, :, y, strip:strip + k], ref[0, :, y, :k]
    elif mut == "phases_swapped":           # rows y and y + 1 belong to neighbouring row phases (neighbouring rows at dilation 1)
        a[0, :, y - 1], a[0, :, y] = ref[0, :, y], ref[0, :, y - 1]
    elif mut == "image_from_next":          # image index off by one
        a[0, :, y] = ref[(0 + 1) % n, :, y] if n > 1 else ref[0, :, y - 1]
    elif mut == "tile_skipped":
        a[n - 1, :, th:2 * th, tw:2 * tw] = np.nan
    elif mut == "channel_block_from_neighbour":
        k = min(tw, w - tw)
        a[0, 8:16, :th, :k] = ref[0, 8:16, :th, tw:tw + k]
    else:
        raise ValueError(mut)
    return a


# ---- the criteria of tests/test_gpu_tower_grids.py, as predicates ---------------------------------------------------------
def same_bits(a, b):
    return mr.same_bits(np.asarray(a), np.asarray(b))


def within(got, ref, rel):
    """max |got - ref| <= rel * max |ref|, False when a value is not finite (a NaN left from the pre-fill)"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    return bool(np.isfinite(got).all()) and float(np.abs(got - ref).max()) <= rel * float(np.abs(ref).max())


def max_rel(got, ref):
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


# ---- the cases of tests/test_gpu_tower_grids.py (shared with the CPU test of the references) ------------------------------
# Streamed blocks, (dil, h, w): three strips, the last a few columns wide; hsub = ceil(h / dil) is 6 or 7, and h is no multiple
# of dil, so the last row phase is one sub-row short.  n in STREAM_N.
STREAM_N = (1, 3)
STREAM_F16 = [(1, 7, 130), (2, 11, 126), (4, 22, 246), (8, 41, 230)]
STREAM_X3 = [(1, 7, 130), (2, 11, 126), (4, 22, 118), (8, 41, 102)]
STREAM_TAIL = (16, 128, 13, 125, 16)          # hk, wk, h_out, w_out, ups: three strips of 60 output columns, 13 rows
CAPS = (8, 16, 24, 64)                        # banded kernels; 0 = the device's CU count is the default grid
