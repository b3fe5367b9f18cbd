"""SN-K4 expressed with torch.nn.functional on CPU — an independent second implementation used to validate the C
oracle, in fp32 (the default; the committed goldens) or, with dtype=torch.float64, as the ground truth
every precision mode and the oracle itself are judged against (`truth`).  The dtype is passed down
explicitly: the suite shares one process, so the process-global default dtype is never touched.  This is not
reference code: the reference has no network arithmetic.
"""
from __future__ import annotations

import contextlib
import os

import numpy as np
import torch
import torch.nn.functional as F

from hobot_stereonet_amd import spec, weights as W


def _t(blob, name, dtype=torch.float32):
    return torch.from_numpy(W.tensor(blob, name).copy()).to(dtype)      # fp32 -> float64 widens exactly


def lrelu(x):
    return F.leaky_relu(x, spec.LRELU_SLOPE)


def res_block(blob, prefix, x, dil):
    dt = x.dtype
    t = lrelu(F.conv2d(x, _t(blob, prefix + ".1.w", dt), _t(blob, prefix + ".1.b", dt), padding=dil, dilation=dil))
    t = F.conv2d(t, _t(blob, prefix + ".2.w", dt), _t(blob, prefix + ".2.b", dt), padding=dil, dilation=dil)
    return lrelu(x + t)


def features(blob, planes):              # planes: (1,3,hp,wp)
    x, dt = planes, planes.dtype
    for i in range(spec.N_DOWN):
        x = F.conv2d(x, _t(blob, f"feat.down{i}.w", dt), _t(blob, f"feat.down{i}.b", dt), stride=2, padding=2)
    for i in range(spec.N_FEAT_RES):
        x = res_block(blob, f"feat.res{i}", x, 1)
    return F.conv2d(x, _t(blob, "feat.out.w", dt), _t(blob, "feat.out.b", dt), padding=1)


def cost_volume(fl, fr, dl):             # (1,C,h,w) -> (1,C,dl,h,w)
    _, c, h, w = fl.shape
    cv = torch.zeros(1, c, dl, h, w, dtype=fl.dtype)
    for d in range(dl):
        if d == 0:
            cv[:, :, 0] = fl - fr
        else:
            cv[:, :, d, :, d:] = fl[..., d:] - fr[..., :-d]
    return cv


def aggregate(blob, fl, fr, dl):
    x, dt = cost_volume(fl, fr, dl), fl.dtype
    for i in range(spec.N_AGG):
        x = lrelu(F.conv3d(x, _t(blob, f"agg.conv{i}.w", dt), _t(blob, f"agg.conv{i}.b", dt), padding=1))
    return F.conv3d(x, _t(blob, "agg.out.w", dt), _t(blob, "agg.out.b", dt), padding=1)[:, 0]   # (1,dl,h,w)


def soft_argmin(cost):                   # (1,dl,h,w) -> (1,h,w)
    p = torch.softmax(-cost, dim=1)
    d = torch.arange(cost.shape[1], dtype=cost.dtype).view(1, -1, 1, 1)
    return (p * d).sum(1)


def refine(blob, disp_up, img, dmax, prefix="ref", moved=None):    # (1,1,hp,wp), (1,3,hp,wp)
    """`moved`: a list that receives dmax * r of this level, BEFORE the relu (what the refinement statistic sums)"""
    dt = disp_up.dtype
    x = torch.cat([disp_up / dmax, img], 1)
    x = lrelu(F.conv2d(x, _t(blob, prefix + ".in.w", dt), _t(blob, prefix + ".in.b", dt), padding=1))
    for i, dil in enumerate(spec.REF_DILATIONS):
        x = res_block(blob, f"{prefix}.res{i}", x, dil)
    r = F.conv2d(x, _t(blob, prefix + ".out.w", dt), _t(blob, prefix + ".out.b", dt), padding=1)
    if moved is not None:
        moved.append((dmax * r)[0, 0].numpy().copy())
    return F.relu(disp_up + dmax * r)


def refine_multi(blob, low, img, dmax, levels, moved=None):
    """Hierarchical refinement (`multi`): level k = levels-1 .. 0 works at 1/2^k resolution on
    the x2 bilinear upsample (values x2) of the level below (the soft-argmin map for the coarsest level), the left image
    average-pooled by 2^k, its own tower weights and D / 2^k as the disparity normalisation."""
    d = low[:, None] * (16.0 / 2 ** levels)          # soft-argmin map in 1/2^levels-resolution pixel units
    per_level = []
    for k in range(levels - 1, -1, -1):
        up = F.interpolate(d, scale_factor=2, mode="bilinear", align_corners=False) * 2.0
        img_k = F.avg_pool2d(img, 2 ** k) if k else img
        d = refine(blob, up, img_k, dmax / 2 ** k, spec.ref_prefix(k), moved)
        per_level.append(d[0, 0].numpy().copy())
    return d, per_level


def forward(blob, in6: np.ndarray, dmax: int, dtype=torch.float32, moved=None):
    """in6 int8 (6,h,w) -> dict(disp (h,w), disp_low, cost, fl, fr, levels), every array of `dtype`: float32 (the
    committed goldens), or float64 with the int8 input / 128 and the fp32 weights widened exactly and no fp32 step.
    `moved`: a list that receives D_k r_k of every refinement level before its relu, over the level's padded map, coarsest
    level first (refine)"""
    _, h, w = in6.shape
    hp, wp = spec.ceil16(h), spec.ceil16(w)
    x = torch.zeros(1, 6, hp, wp, dtype=dtype)
    if dtype == torch.float32:
        x[0, :, :h, :w] = torch.from_numpy(in6.astype(np.float32) / 128.0)
    else:
        x[0, :, :h, :w] = torch.from_numpy(in6.astype(np.int32)).to(dtype) / 128.0       # exact: |in6| <= 128, / 2^7
    with torch.no_grad():
        fl = features(blob, x[:, :3])
        fr = features(blob, x[:, 3:])
        cost = aggregate(blob, fl, fr, dmax // 16)
        low = soft_argmin(cost)
        levels = spec.levels_of(blob.size)
        per_level = []
        if levels == 1:
            up = F.interpolate(low[:, None], scale_factor=16, mode="bilinear", align_corners=False) * 16.0
            disp = refine(blob, up, x[:, :3], dmax, moved=moved)
        else:
            disp, per_level = refine_multi(blob, low, x[:, :3], dmax, levels, moved)
    return {"levels": per_level, "disp": disp[0, 0, :h, :w].numpy().copy(), "disp_low": low[0].numpy().copy(),
            "cost": cost[0].numpy().copy(), "fl": fl[0].numpy().copy(), "fr": fr[0].numpy().copy()}


def env_threads() -> int:
    """The thread count the environment grants this process (OMP_NUM_THREADS, else the CPUs it may run on, 16 at the
    most: the convolutions here do not scale further) — never the machine's CPU count, which on a shared box is many
    times what one job may use."""
    try:
        n = int(os.environ.get("OMP_NUM_THREADS", "0"))
    except ValueError:
        n = 0
    return n if n > 0 else max(1, min(16, len(os.sched_getaffinity(0))))


@contextlib.contextmanager
def torch_threads(n=None):
    before = torch.get_num_threads()
    torch.set_num_threads(n or env_threads())
    try:
        yield
    finally:
        torch.set_num_threads(before)


def truth(blob, in6: np.ndarray, dmax: int, moved=None):
    """The float64 ground truth of one input: forward() in float64 -> dict(disp, disp_low, cost, fl, fr, levels)."""
    with torch_threads():
        return forward(blob, in6, dmax, torch.float64, moved)
