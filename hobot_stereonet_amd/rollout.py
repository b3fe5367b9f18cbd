"""The trajectory rollout, from the plan to a velocity command: the parameters of ``sn_rollout`` (include/stereonet_hip.h), the
refusals of the C side in its words, the host tables and the pose quantisation restated in Python (the library's own are what a
twin is fed: two libms may differ by an ulp), a vectorised numpy twin of the integer walk, a plain loop over Python integers
written from the header against which the twin is checked, the footprint and window helpers, the parameter file of the tools and
the node, and what ``filelist --rollout`` writes.

The inputs are a cost grid as ``sn_inflate_grid`` writes it (0 free, 1..252 graded, 253 inscribed, 254 lethal, 255 unknown) and
the potential ``sn_navfn`` made of it.  Sample ``s = iv * nw + iw``; positions are in 1/256 cell, headings in 1/65536 turn.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Sequence, Tuple

import numpy as np

from . import paramfile

MAX_STEPS = 64                      # SN_ROLLOUT_MAX_STEPS
MAX_POINTS = 64                     # SN_ROLLOUT_MAX_POINTS
MAX_SIDE = 64                       # SN_ROLLOUT_MAX_SIDE: nv, nw
MAX_GRID_SIDE = 4096                # gw, gh
MAX_AREA = 1 << 20                  # gw * gh, sn_navfn's
INF = 0xFFFFFFFF                    # SN_NAV_INF
UNKNOWN_OK = 1                      # SN_ROLLOUT_UNKNOWN_OK
NO_VALID = 1                        # SN_ROLLOUT_NO_VALID
VALID, OUT_OF_WINDOW, COLLISION, NO_ROUTE = 0, 1, 2, 3
REASONS = ("valid", "out_of_window", "collision", "no_route")
BEST = ("flags", "s_best", "score_lo", "score_hi", "valid", "collided", "no_route", "out_of_window")
WAVE = 64                           # a wave of k_rollout_eval covers 64 (step, point) pairs a pass
GROUP = 4                           # kRoWaves: a workgroup of k_rollout_eval covers 4 samples of one iw
BEST_THREADS = 256                  # kRoBestThreads: k_rollout_best strides the samples of a map by this
TWO_PI = 6.283185307179586
MAX_THETA = 1048576.0
MAX_REACH = 1 << 21


@dataclasses.dataclass
class RolloutParams:
    """sn_rollout_params, and for the tools the footprint (points in metres, robot frame) and the pose {x, y, yaw} in the grid's
    frame with the grid's origin at (0, 0) (None: the start cell's centre, yaw 0; the node takes the pose from the costmap), and
    for the node acc = (acc_v, acc_w, dt): what window_from_velocity makes of SetVelocity's (v, w) (None: every sample)."""
    cell_m: float = 0.05
    v_min: float = 0.0
    v_max: float = 0.5
    nv: int = 11
    w_min: float = -1.0
    w_max: float = 1.0
    nw: int = 21
    sim_time_s: float = 1.5
    steps: int = 15
    lethal_cost: int = 254
    centre_lethal_cost: int = 253
    unknown_cost: int = 0
    flags: int = 0
    w_goal: int = 1
    w_occ: int = 1
    footprint: Tuple[Tuple[float, float], ...] = ()
    pose: Optional[Tuple[float, float, float]] = None
    acc: Optional[Tuple[float, float, float]] = None


_FLOATS = ("cell_m", "v_min", "v_max", "w_min", "w_max", "sim_time_s")
_INTS = ("nv", "nw", "steps", "lethal_cost", "centre_lethal_cost", "unknown_cost", "flags", "w_goal", "w_occ")


def _f32(v) -> float:
    return float(np.float32(v))


def footprint_array(p: RolloutParams, footprint=None) -> np.ndarray:
    """the footprint as float32 (nf, 2): `footprint`, or the parameter block's own"""
    fp = p.footprint if footprint is None else footprint
    return np.ascontiguousarray(np.asarray(fp, np.float32).reshape(-1, 2))


def check(p: RolloutParams, footprint=None) -> Optional[str]:
    """None, or why sn_rollout_tables refuses these parameters and this footprint (the tables' own range test is tables')"""
    vals = [_f32(getattr(p, k)) for k in _FLOATS]
    if not all(math.isfinite(v) for v in vals):
        return "every parameter must be finite"
    if not vals[0] > 0:
        return "cell_m must be positive"
    if not vals[5] > 0:
        return "sim_time_s must be positive"
    if vals[2] < vals[1] or vals[4] < vals[3]:
        return "v_min <= v_max and w_min <= w_max are required"
    if not (1 <= p.nv <= MAX_SIDE and 1 <= p.nw <= MAX_SIDE):
        return "nv and nw must be 1..64"
    if not 1 <= p.steps <= MAX_STEPS:
        return "steps must be 1..64"
    if not 1 <= p.lethal_cost <= 255:
        return "lethal_cost must be 1..255"
    if not 1 <= p.centre_lethal_cost <= 255:
        return "centre_lethal_cost must be 1..255"
    if not 0 <= p.unknown_cost <= 252:
        return "unknown_cost must be 0..252"
    if p.flags & ~UNKNOWN_OK:
        return "flags has bits other than SN_ROLLOUT_UNKNOWN_OK"
    if not (0 <= p.w_goal <= 32767 and 0 <= p.w_occ <= 32767):
        return "w_goal and w_occ must be 0..32767"
    if p.w_goal == 0 and p.w_occ == 0:
        return "w_goal and w_occ must not both be 0"
    fp = footprint_array(p, footprint)
    if fp.shape[0] > MAX_POINTS:
        return "nf must be 0..64"
    if not np.all(np.isfinite(fp)):
        return "the footprint must be finite"
    return None


def _lattice(lo: float, hi: float, count: int) -> np.ndarray:
    lo, hi = _f32(lo), _f32(hi)
    if count == 1:
        return np.array([lo], np.float64)
    return lo + np.arange(count, dtype=np.float64) * ((hi - lo) / (count - 1))


def velocity(p: RolloutParams, s: int) -> Tuple[float, float]:
    """(v, w) of sample s: sn_rollout_velocity"""
    if check(p, ()) or not 0 <= s < p.nv * p.nw:
        raise ValueError("bad parameters or s outside 0..S-1")
    return float(_lattice(p.v_min, p.v_max, p.nv)[s // p.nw]), float(_lattice(p.w_min, p.w_max, p.nw)[s % p.nw])


def _llrint(a) -> np.ndarray:
    return np.rint(a).astype(np.int64)      # ties to even, as llrint in the default rounding mode


def tables(p: RolloutParams, footprint=None):
    """The header's tables restated: -> (centres int32 (S, T+1, 3), offsets int32 (nw, T+1, nf, 2)).  ValueError where
    sn_rollout_tables refuses.  Within 1 of the library's per entry (sin and cos)."""
    why = check(p, footprint)
    if why:
        raise ValueError(why)
    fp = footprint_array(p, footprint).astype(np.float64)
    nf, T = fp.shape[0], p.steps
    k256 = 256.0 / _f32(p.cell_m)
    v, w = _lattice(p.v_min, p.v_max, p.nv), _lattice(p.w_min, p.w_max, p.nw)
    tau = (_f32(p.sim_time_s) * np.arange(T + 1, dtype=np.float64)) / T
    th = w[:, None] * tau[None, :]                                               # (nw, T+1)
    if not np.all(np.abs(th) <= MAX_THETA):
        raise ValueError("the heading turns by more than 2^20 rad")
    c, s = np.cos(th), np.sin(th)
    ox = (c[..., None] * fp[:, 0] - s[..., None] * fp[:, 1]) * k256              # (nw, T+1, nf)
    oy = (s[..., None] * fp[:, 0] + c[..., None] * fp[:, 1]) * k256
    if not (np.all(np.abs(ox) <= MAX_REACH) and np.all(np.abs(oy) <= MAX_REACH)):
        raise ValueError("a footprint point lies more than 2^21 / 256 cells from the centre")
    offsets = np.stack([_llrint(ox), _llrint(oy)], -1)
    vv, ww = v[:, None, None], w[None, :, None]                                   # (nv, nw, T+1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = vv / ww
        x = np.where(np.abs(th)[None] < 1e-6, vv * tau, r * s[None])
        y = np.where(np.abs(th)[None] < 1e-6, ((vv * tau) * th[None]) / 2.0, r * (1.0 - c[None]))
    xs, ys = x * k256, y * k256
    if not (np.all(np.abs(xs) <= MAX_REACH) and np.all(np.abs(ys) <= MAX_REACH)):
        raise ValueError("an arc reaches more than 2^21 / 256 cells from its start")
    bam = _llrint((th / TWO_PI) * 65536.0) & 0xFFFF
    centres = np.stack([_llrint(xs), _llrint(ys), np.broadcast_to(bam[None], xs.shape)], -1)      # (nv, nw, T+1, 3)
    if nf:
        reach = centres[..., None, :2] + offsets[None]
        if np.any(np.abs(reach) > MAX_REACH):
            raise ValueError("a footprint point reaches more than 2^21 / 256 cells from the arc's start")
    return centres.reshape(p.nv * p.nw, T + 1, 3).astype(np.int32), offsets.astype(np.int32)


def pose_q(cell_m: float, origin_x_m: float, origin_y_m: float, pose) -> np.ndarray:
    """sn_rollout_pose_q restated: pose {x, y, yaw} -> int32 (5,) = {px, py, cq, sq, yaw_bam}; ValueError where it refuses"""
    cell = _f32(cell_m)
    x, y, yaw = (float(v) for v in pose)
    ok = math.isfinite(cell) and cell > 0 and all(math.isfinite(v) for v in (origin_x_m, origin_y_m, x, y, yaw)) and abs(yaw) <= MAX_THETA
    if not ok:
        raise ValueError("a pose or an origin that is not finite, or a bad cell_m")
    k256 = 256.0 / cell
    fx, fy = (x - float(origin_x_m)) * k256, (y - float(origin_y_m)) * k256
    if not (abs(fx) <= 2.0 ** 30 and abs(fy) <= 2.0 ** 30):
        raise ValueError("the pose lies more than 2^30 / 256 cells from the origin")
    return np.array([round(fx), round(fy), round(math.cos(yaw) * 2.0 ** 30), round(math.sin(yaw) * 2.0 ** 30),
                     round((yaw / TWO_PI) * 65536.0) & 0xFFFF], np.int32)


def _prepare(cost, potential, poses_q, window, p, centres, offsets):
    why = check(p, ())
    if why:
        raise ValueError(why)
    c = np.asarray(cost, np.uint8)
    c = c[None] if c.ndim == 2 else c
    if c.ndim != 3 or not (1 <= c.shape[1] <= MAX_GRID_SIDE and 1 <= c.shape[2] <= MAX_GRID_SIDE):
        raise ValueError("gw and gh must be 1..4096")
    if c.shape[1] * c.shape[2] > MAX_AREA:
        raise ValueError("gw * gh must be at most 2^20")
    P = np.asarray(potential, np.uint32).reshape(c.shape)
    q = np.asarray(poses_q, np.int64).reshape(-1, 5)
    win = None if window is None else np.asarray(window, np.int64).reshape(-1, 4)
    if q.shape[0] != c.shape[0] or (win is not None and win.shape[0] != c.shape[0]):
        raise ValueError("one pose (and one window) per map is needed")
    if np.any(np.abs(q[:, :2]) > 1 << 30) or np.any(np.abs(q[:, 2:4]) > 1 << 30):
        raise ValueError("poses_q is not what sn_rollout_pose_q writes")
    S, T1 = p.nv * p.nw, p.steps + 1
    cen = np.asarray(centres, np.int64)
    off = np.asarray(offsets, np.int64)
    if cen.shape != (S, T1, 3) or off.ndim != 4 or off.shape[:2] != (p.nw, T1) or off.shape[3] != 2 or off.shape[2] > MAX_POINTS:
        raise ValueError("centres (S, T+1, 3) and offsets (nw, T+1, nf, 2) are needed")
    return c, P, q, win, cen, off


def _rotate(q, qx, qy):
    """the contract's X and Y of points {qx, qy} (int64 arrays) under the pose q = {px, py, cq, sq, ...} (Python ints)"""
    px, py, cq, sq = (int(v) for v in q[:4])
    return px + ((cq * qx - sq * qy + (1 << 29)) >> 30), py + ((sq * qx + cq * qy + (1 << 29)) >> 30)


def reference(cost, potential, poses_q, window, p: RolloutParams, centres, offsets):
    """cost uint8 (gh, gw) or (n, gh, gw), potential uint32 of that shape, poses_q (n, 5), window (n, 4) or None, the library's
    tables -> (samples uint32 (n, S, 2), best uint32 (n, 8), traj int32 (n, T+1, 3): zeros for a map without a valid sample,
    which the call does not write)."""
    c, P, q, win, cen, off = _prepare(cost, potential, poses_q, window, p, centres, offsets)
    n, gh, gw = c.shape
    S, T1, nf = p.nv * p.nw, p.steps + 1, off.shape[2]
    iv, iw = np.divmod(np.arange(S), p.nw)
    qx = np.concatenate([cen[:, :, None, 0], cen[:, :, None, 0] + off[iw, :, :, 0]], 2)      # (S, T+1, nf+1), point 0 = the centre
    qy = np.concatenate([cen[:, :, None, 1], cen[:, :, None, 1] + off[iw, :, :, 1]], 2)
    thr = np.full(nf + 1, p.lethal_cost, np.int64)
    thr[0] = p.centre_lethal_cost
    samples = np.zeros((n, S, 2), np.uint32)
    best = np.zeros((n, 8), np.uint32)
    traj = np.zeros((n, T1, 3), np.int32)
    for k in range(n):
        X, Y = _rotate(q[k], qx, qy)
        cx, cy = X >> 8, Y >> 8
        inside = (cx >= 0) & (cx < gw) & (cy >= 0) & (cy < gh)
        cc = c[k][np.clip(cy, 0, gh - 1), np.clip(cx, 0, gw - 1)].astype(np.int64)
        unknown = cc == 255
        price = np.where(unknown, p.unknown_cost, cc)
        hit = ~inside | np.where(unknown, not p.flags & UNKNOWN_OK, cc >= thr)
        hit_t = hit.any(2)                                                      # (S, T+1)
        collided = hit_t.any(1)
        step = np.where(collided, hit_t.argmax(1), 0)
        occ = np.where(hit, 0, price).max((1, 2))
        g = P[k][np.clip(cy[:, -1, 0], 0, gh - 1), np.clip(cx[:, -1, 0], 0, gw - 1)].astype(np.int64)
        inwin = np.ones(S, bool) if win is None else (iv >= win[k, 0]) & (iv <= win[k, 1]) & (iw >= win[k, 2]) & (iw <= win[k, 3])
        reason = np.where(~inwin, OUT_OF_WINDOW, np.where(collided, COLLISION, np.where(g == INF, NO_ROUTE, VALID)))
        valid = reason == VALID
        samples[k, :, 0] = np.where(valid, g, INF)
        samples[k, :, 1] = np.where(valid, occ, 0) | reason << 8 | np.where(reason == COLLISION, step, 0) << 16
        counts = [int((reason == r).sum()) for r in (VALID, COLLISION, NO_ROUTE, OUT_OF_WINDOW)]
        if valid.any():
            score = p.w_goal * g + p.w_occ * occ                                # < 2^48: int64 holds it
            key = np.where(valid, score << 16 | np.arange(S), np.iinfo(np.int64).max)
            sb = int(key.argmin())
            best[k] = [0, sb, int(score[sb]) & 0xFFFFFFFF, int(score[sb]) >> 32] + counts
            tx, ty = _rotate(q[k], cen[sb, :, 0], cen[sb, :, 1])
            traj[k] = np.stack([tx, ty, (int(q[k, 4]) + cen[sb, :, 2]) & 0xFFFF], 1)
        else:
            best[k] = [NO_VALID, INF, INF, INF] + counts
    return samples, best, traj


def loop_reference(cost, potential, pose_q5, window, p: RolloutParams, centres, offsets):
    """The header again for ONE map, over Python integers, one sample, step and point at a time; shares nothing with reference.
    -> (samples (S, 2), best (8,), traj (T+1, 3) or None) as lists of Python ints.  Slow: small cases only."""
    c = np.asarray(cost, np.uint8).tolist()
    P = np.asarray(potential, np.uint32).tolist()
    gh, gw = len(c), len(c[0])
    px, py, cq, sq, yaw = (int(v) for v in pose_q5)
    cen, off = np.asarray(centres).tolist(), np.asarray(offsets).tolist()
    T = p.steps
    nf = len(off[0][0])

    def place(x, y):
        return px + ((cq * x - sq * y + (1 << 29)) >> 30), py + ((sq * x + cq * y + (1 << 29)) >> 30)

    samples, counts, best_key = [], [0, 0, 0, 0], None
    for s in range(p.nv * p.nw):
        iv, iw = divmod(s, p.nw)
        if window is not None and not (window[0] <= iv <= window[1] and window[2] <= iw <= window[3]):
            samples.append([INF, OUT_OF_WINDOW << 8])
            counts[3] += 1
            continue
        step, occ = None, 0
        for t in range(T + 1):
            for f in range(nf + 1):
                x, y = cen[s][t][0], cen[s][t][1]
                if f:
                    x, y = x + off[iw][t][f - 1][0], y + off[iw][t][f - 1][1]
                X, Y = place(x, y)
                cx, cy = X >> 8, Y >> 8
                if not (0 <= cx < gw and 0 <= cy < gh):
                    hit = True
                elif c[cy][cx] == 255:
                    hit = not p.flags & UNKNOWN_OK
                    occ = occ if hit else max(occ, p.unknown_cost)
                else:
                    hit = c[cy][cx] >= (p.lethal_cost if f else p.centre_lethal_cost)
                    occ = occ if hit else max(occ, c[cy][cx])
                if hit and step is None:
                    step = t
            if step is not None:
                break
        if step is not None:
            samples.append([INF, COLLISION << 8 | step << 16])
            counts[1] += 1
            continue
        X, Y = place(cen[s][T][0], cen[s][T][1])
        g = P[Y >> 8][X >> 8]
        if g == INF:
            samples.append([INF, NO_ROUTE << 8])
            counts[2] += 1
            continue
        samples.append([g, occ])
        counts[0] += 1
        key = (p.w_goal * g + p.w_occ * occ, s)
        best_key = key if best_key is None or key < best_key else best_key
    if best_key is None:
        return samples, [NO_VALID, INF, INF, INF] + counts, None
    score, sb = best_key
    traj = [list(place(cen[sb][t][0], cen[sb][t][1])) + [(yaw + cen[sb][t][2]) & 0xFFFF] for t in range(T + 1)]
    return samples, [0, sb, score & 0xFFFFFFFF, score >> 32] + counts, traj


# ---- helpers of the caller -----------------------------------------------------------------------------------------------------------
def rectangle_footprint(length_m: float, width_m: float, spacing_m: float) -> np.ndarray:
    """The outline of a length x width rectangle centred on the robot (x ahead), sampled so that neighbouring points lie at most
    spacing_m apart: each side in ceil(side / spacing) equal parts, every corner once -> float32 (nf, 2), counter-clockwise from
    the front left corner.  ValueError where that needs more than MAX_POINTS points or an argument is not positive and finite."""
    if not all(math.isfinite(v) and v > 0 for v in (length_m, width_m, spacing_m)):
        raise ValueError("length_m, width_m and spacing_m must be positive and finite")
    na, nb = math.ceil(length_m / spacing_m - 1e-9), math.ceil(width_m / spacing_m - 1e-9)
    if 2 * (na + nb) > MAX_POINTS:
        raise ValueError(f"{2 * (na + nb)} points: more than {MAX_POINTS}")
    hx, hy = length_m / 2.0, width_m / 2.0
    pts = [(hx - length_m * i / na, hy) for i in range(na)] + [(-hx, hy - width_m * i / nb) for i in range(nb)] + \
          [(-hx + length_m * i / na, -hy) for i in range(na)] + [(hx, -hy + width_m * i / nb) for i in range(nb)]
    return np.array(pts, np.float32)


def window_from_velocity(p: RolloutParams, v: float, w: float, acc_v: float, acc_w: float, dt: float) -> np.ndarray:
    """The dynamic window: the lattice samples the motors reach from (v, w) within dt at accelerations acc_v (m/s^2) and acc_w
    (rad/s^2) -> int32 (4,) = {iv_lo, iv_hi, iw_lo, iw_hi}.  An axis on which no sample lies in reach keeps the one nearest to
    the present velocity (the lower on a tie), so the window is never empty."""
    if check(p, ()):
        raise ValueError(check(p, ()))
    if not all(math.isfinite(x) for x in (v, w, acc_v, acc_w, dt)) or acc_v < 0 or acc_w < 0 or dt < 0:
        raise ValueError("v, w, acc_v, acc_w and dt must be finite, the last three not negative")

    def axis(lattice, at, reach):
        inside = np.nonzero((lattice >= at - reach) & (lattice <= at + reach))[0]
        if inside.size:
            return int(inside[0]), int(inside[-1])
        near = int(np.abs(lattice - at).argmin())
        return near, near

    return np.array(axis(_lattice(p.v_min, p.v_max, p.nv), v, acc_v * dt) + axis(_lattice(p.w_min, p.w_max, p.nw), w, acc_w * dt), np.int32)


# ---- the parameter file: one `key value` per line, `#` comments, as navfn.py's; `point x y` lines are the footprint, `pose x y yaw`
# the tools' pose, `acc acc_v acc_w dt` the node's window ------------------------------------------------------------------------------------------------------------------------
_FILE = paramfile.spec(_FLOATS, _INTS, point=paramfile.Key(2, float, repeat=True), pose=paramfile.Key(3), acc=paramfile.Key(3))


def save_params(path: str, p: RolloutParams) -> None:
    paramfile.write(path, "trajectory rollout: velocities in m/s and rad/s; flags 1 = unknown cells are priced at unknown_cost; one `point x y`\n"
                    "# line per footprint point (metres, robot frame); pose x y yaw in the grid's frame; acc acc_v acc_w dt: the node's window",
                    _FILE, [(k, getattr(p, k)) for k in _FLOATS + _INTS] +
                    [("point", xy) for xy in np.asarray(p.footprint, np.float64).reshape(-1, 2).tolist()] +
                    [(k, getattr(p, k)) for k in ("pose", "acc") if getattr(p, k) is not None])


def load_params(path: str) -> RolloutParams:
    """A key that is missing keeps RolloutParams' default; an unknown or repeated key (but `point`), or a wrong number of values,
    is an error."""
    got = paramfile.read(path, _FILE)
    return RolloutParams(footprint=tuple(got.pop("point", ())), **got)


# ---- what `filelist --rollout` writes ------------------------------------------------------------------------------------------------
def write_rollout(path: str, v: float, w: float, best, traj) -> None:
    """`cmd v w`, `best` and its eight words, then one `X Y heading` line per step of the trajectory (none without a valid sample)"""
    with open(path, "w") as f:
        f.write(f"cmd {v!r} {w!r}\n")
        f.write("best " + " ".join(str(int(x)) for x in best) + "\n")
        if not int(best[0]) & NO_VALID:
            for x, y, a in np.asarray(traj).tolist():
                f.write(f"{x} {y} {a}\n")
