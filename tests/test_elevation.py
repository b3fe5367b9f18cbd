"""sn_elevation on the host: the vectorised twin (hobot_stereonet_amd/elevation.py) against the plain loop over Python integers
that was written from the header, byte for byte; n pushes against one push of n; interleaved streams; scrolling by a cell, by
mw - 1 and by more than a window; alpha 256 against 64, up and down; the accumulators at the declared integer limits; the
refused parameter sets; the parameter file.  No GPU and no tolerance anywhere."""
import dataclasses
import math

import numpy as np
import pytest

from hobot_stereonet_amd import elevation as el
from hobot_stereonet_amd.elevation import ElevationParams
from hobot_stereonet_amd.pointcloud import Camera

W, H = 24, 16
CAM = Camera(fx=14.0, fy=14.0, baseline_mm=120.0)
P = ElevationParams(mw=13, mh=9, cell_m=0.5, z_min_m=-1.0, z_max_m=1.5, range_max_m=6.0, min_points=2, alpha=64, max_step_mm=80,
                    radius=1)
NAMES = ("trav", "hi", "lo", "rise", "stats")


def _q(p, poses):
    return np.stack([el.pose_q(p, x) for x in np.asarray(poses, np.float64).reshape(-1, 3)])


def _same(a, b):
    return [n for n, x, y in zip(NAMES, a, b) if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes()]


def _flat(height_m, wall_m=30.0, w=W, h=H, cam=CAM):
    """a smooth floor `height_m` below the camera (and a wall far away): every pixel valid"""
    return el.terrain_map(w, h, cam, height_m, wall_m, rough_m=0.0, holes=0.0)


@pytest.mark.parametrize("seed,radius,mw,mh", [(1, 1, 13, 9), (2, 2, 7, 12), (3, 3, 1, 1), (4, 3, 5, 3), (5, 1, 1, 7)])
def test_the_twin_equals_the_plain_loop_on_seeded_clips(seed, radius, mw, mh):
    p = dataclasses.replace(P, radius=radius, mw=mw, mh=mh)
    poses, raw = el.synthetic_clip(p, W, H, CAM, 6, seed=seed)
    q = _q(p, poses)
    twin, loop = el.Reference(p, 2), el.LoopReference(p, 2)
    ids = [0, 1, 1, 0, 0, 1]
    a, b = twin.push(q, raw, CAM, stream_of=ids), loop.push(q, raw, CAM, stream_of=ids)
    assert not _same(a, b)
    if mw * mh > 50:      # the clip is worth something: cells are born, blended both ways and scrolled away, and all three verdicts appear
        br = twin.frames
        assert sum(f["born"] for f in br) and sum(f["up"] for f in br) and sum(f["down"] for f in br) and sum(f["scrolled"] for f in br)
        assert {-1, 0, 100} <= set(np.unique(a[0]).tolist())
        assert a[4][:, 3].min() > 0 and (a[4][:, 2] < a[4][:, 0]).any()


def test_the_twin_equals_the_plain_loop_with_mounts_and_a_step():
    p = dataclasses.replace(P, cell_m=0.25, min_points=1)
    cam = dataclasses.replace(CAM, step=2, z_min_m=0.3, z_max_m=8.0)
    poses, raw = el.synthetic_clip(p, W, H, cam, 3, seed=9)
    from hobot_stereonet_amd import obstacles
    mounts = np.asarray([obstacles.mount(0.1, 0.2, (0.1, 0.0, 0.5)), obstacles.mount(-0.2, 0.1, (0.0, 0.1, 0.4)), (np.nan,) * 12], np.float32)
    q = _q(p, poses)
    a, b = el.Reference(p).push(q, raw, cam, mounts), el.LoopReference(p).push(q, raw, cam, mounts)
    assert not _same(a, b)
    assert a[4][0, 2] > 0 and a[4][2, 2] == 0 and a[4][2, 3] == 0      # a mount that is not finite fuses nothing


def test_the_accumulators_at_the_declared_integer_limits():
    """samples given directly: heights on and beyond z_min / z_max = -+32 m, NaN and infinities in every coordinate, subs on both
    sides of 2^30, the range on and past range_max_m, and a pose on the quantiser's limit with yaw 0, pi/2 and pi"""
    cell = 2.0 ** -20      # k256 = 2^28: xb = 3.99 m is 1.07e9 subs, just under 2^30, and 4 m is 2^30
    p = ElevationParams(mw=9, mh=7, cell_m=cell, z_min_m=-32.0, z_max_m=32.0, range_max_m=5.0, min_points=1, alpha=256, max_step_mm=32767,
                        radius=3)
    assert el.units(p).zmin_mm == -32000 and el.units(p).zmax_mm == 32000
    f = np.float32
    just_under = np.nextafter(f(4.0), f(0.0))
    xs = [0.0, 1e-7, -1e-7, just_under, 4.0, -just_under, -4.0, 5.0, np.nextafter(f(5.0), f(6.0)), np.nan, np.inf, -np.inf, 3e-6, -3e-6]
    zs = [0.0, 32.0, np.nextafter(f(32.0), f(33.0)), -32.0, np.nextafter(f(-32.0), f(-33.0)), 32.0009, np.nan, np.inf, -np.inf, 1e30, -0.0005]
    xb, yb, zb = (a.astype(np.float32).reshape(-1) for a in np.meshgrid(xs, xs, zs, indexing="ij"))
    lim = 2.0 ** 30 / el.units(p).k256
    used = 0
    for pose in [(0.0, 0.0, 0.0), (lim, -lim, 0.0), (-lim, lim, math.pi / 2), (lim, lim, math.pi), (1e-6, 2e-6, 0.7)]:
        q = el.pose_q(p, pose)
        a, b = el.accumulate(p, q, xb, yb, zb), el.LoopReference(p).accumulate(q, xb, yb, zb)
        for x, y in zip(a, b):
            assert np.array_equal(x, np.asarray(y, np.int64)), pose
        used += int(a[0].sum())
        assert a[1][a[0] > 0].max() <= 32000 and a[2][a[0] > 0].min() >= -32000
    assert used > 0
    with pytest.raises(ValueError):
        el.pose_q(p, (np.nextafter(lim, 2 * lim), 0.0, 0.0))
    with pytest.raises(ValueError):
        el.pose_q(p, (0.0, np.nan, 0.0))


def test_n_pushes_equal_one_push_of_n_and_streams_do_not_mix():
    poses, raw = el.synthetic_clip(P, W, H, CAM, 6, seed=11)
    q = _q(P, poses)
    whole = el.Reference(P).push(q, raw, CAM)
    single = el.Reference(P)
    parts = [single.push(q[k:k + 1], raw[k:k + 1], CAM) for k in range(6)]
    assert not _same([np.concatenate(x) for x in zip(*parts)], whole)
    # two streams interleaved in one push: each equals its own clip pushed alone
    ids = np.array([0, 1, 0, 0, 1, 1])
    both = el.Reference(P, 2).push(q, raw, CAM, stream_of=ids)
    for s in (0, 1):
        alone = el.Reference(P).push(q[ids == s], raw[ids == s], CAM)
        assert not _same([x[ids == s] for x in both], alone), s
    # a reset stream starts afresh
    r = el.Reference(P, 2)
    r.push(q[:3], raw[:3], CAM, stream_of=[0, 1, 0])
    r.reset(1)
    again = r.push(q[3:], raw[3:], CAM, stream_of=[1, 1, 1])
    assert not _same(again, el.Reference(P).push(q[3:], raw[3:], CAM))


@pytest.mark.parametrize("shift", [1, P.mw - 1, P.mw, 3 * P.mw + 2])
def test_scrolling_keeps_exactly_the_cells_both_windows_hold(shift):
    """the second frame sees nothing (an all-zero map), so what it reports is the first frame's cells, moved: the world cells
    that both windows hold keep their heights, every other cell is unknown.  Along x, and the same along y."""
    for axis in (0, 1):
        size = P.mw if axis == 0 else P.mh
        step = min(shift, 4 * size)
        pose1 = [0.0, 0.0, 0.0]
        pose1[axis] = step * P.cell_m
        q = _q(P, [(0.0, 0.0, 0.0), pose1])
        raw = np.stack([_flat(0.5), np.zeros((H, W), np.int32)])
        for ref in (el.Reference(P), el.LoopReference(P)):
            trav, hi, lo, rise, stats = ref.push(q, raw, CAM)
            assert stats[1, 2] == 0 and stats[1, 3] == 0 and stats[0, 0] > 0
            want_hi, want_lo = np.full_like(hi[0], el.UNKNOWN), np.full_like(lo[0], el.UNKNOWN)
            if step < size:
                if axis == 0:
                    want_hi[:, :size - step], want_lo[:, :size - step] = hi[0][:, step:], lo[0][:, step:]
                else:
                    want_hi[:size - step], want_lo[:size - step] = hi[0][step:], lo[0][step:]
            assert np.array_equal(hi[1], want_hi) and np.array_equal(lo[1], want_lo), (axis, shift)
            assert stats[1, 0] == (want_hi != el.UNKNOWN).sum()
            if step < size - 1:
                assert stats[1, 0] > 0      # the check is not empty


def test_alpha_256_replaces_and_64_blends_a_quarter_up_and_down():
    q = _q(P, [(0.0, 0.0, 0.0)] * 3)
    for first, second in ((0.5, 0.3), (0.3, 0.5)):      # the floor rises by 0.2 m, then falls
        raw = np.stack([_flat(first), _flat(second), _flat(second)])
        p256, p64 = dataclasses.replace(P, alpha=256), dataclasses.replace(P, alpha=64)
        alone = el.Reference(P).push(q[:1], raw[1:2], CAM)
        a = el.Reference(p256).push(q, raw, CAM)
        b = el.Reference(p64).push(q, raw, CAM)
        both = (a[1][0] != el.UNKNOWN) & (alone[1][0] != el.UNKNOWN)
        assert both.sum() > 10
        assert np.array_equal(a[1][1][both], alone[1][0][both]) and np.array_equal(a[2][1][both], alone[2][0][both])
        for plane in (1, 2):
            old, new, got1, got2 = (x.astype(np.int64)[both] for x in (b[plane][0], alone[plane][0], b[plane][1], b[plane][2]))
            want1 = old + (((new - old) * 64 + 128) >> 8)
            assert np.array_equal(got1, want1) and np.array_equal(got2, want1 + (((new - want1) * 64 + 128) >> 8))
            assert (np.sign(got1 - old) == np.sign(second * -1 + first)).all()      # a floor that comes nearer to the camera rises


def test_the_verdict_of_a_step_and_of_a_slope():
    """planes given directly: a 60 mm kerb is lethal on both sides of its edge within `radius` and nowhere else; a slope whose
    rise over the neighbourhood stays under max_step_mm is free; unknown neighbours and the window's border do not count"""
    p = dataclasses.replace(P, mw=12, mh=8, max_step_mm=59)
    hi = np.zeros((8, 12), np.int16)
    hi[:, 6:] = 60
    for radius in (1, 2, 3):
        trav, rise = el.verdict(dataclasses.replace(p, radius=radius), hi, hi)
        want = np.zeros((8, 12), np.int8)
        want[:, 6 - radius:6 + radius] = 100
        assert np.array_equal(trav, want) and rise.max() == 60
    slope = (np.arange(12, dtype=np.int16) * 19)[None, :].repeat(8, 0)      # 19 mm a cell, and a spread of 2 mm inside each cell
    trav, rise = el.verdict(p, slope + 2, slope)
    assert not trav.any() and (rise == 19 + 2).all()                        # radius 1: the neighbour one cell up the slope
    trav, rise = el.verdict(dataclasses.replace(p, radius=3), slope + 2, slope)
    assert not trav.any() and rise.max() == 3 * 19 + 2 == p.max_step_mm
    trav, rise = el.verdict(dataclasses.replace(p, radius=3, max_step_mm=58), slope + 2, slope)
    assert (trav == 100).all()                                              # every cell has a neighbour three cells away
    hole = slope.copy()
    hole[3, 5] = el.UNKNOWN
    trav, rise = el.verdict(p, hole, hole)
    assert trav[3, 5] == -1 and rise[3, 5] == 0 and (np.delete(trav.reshape(-1), 3 * 12 + 5) == 0).all()


BAD = [dict(mw=0), dict(mh=4097), dict(cell_m=0.0), dict(cell_m=float("nan")), dict(z_min_m=-32.5), dict(z_max_m=32.5),
       dict(z_min_m=1.0, z_max_m=0.5), dict(range_max_m=0.0), dict(range_max_m=float("inf")), dict(min_points=0), dict(alpha=0),
       dict(alpha=257), dict(max_step_mm=0), dict(max_step_mm=32768), dict(radius=0), dict(radius=4), dict(flags=1),
       dict(base_from_cam=(float("nan"),) + (0.0,) * 11)]


@pytest.mark.parametrize("kw", BAD, ids=[str(k) for k in BAD])
def test_refused_parameter_sets(kw):
    assert el.check(P) is None
    p = dataclasses.replace(P, **kw)
    assert el.check(p)
    with pytest.raises(ValueError):
        el.Reference(p)


def test_the_parameter_file_round_trip(tmp_path):
    from hobot_stereonet_amd import obstacles
    p = dataclasses.replace(P, cell_m=0.1, z_min_m=-0.7, range_max_m=1 / 3, base_from_cam=obstacles.mount(0.1, 0.3, (0.1, 0.2, 0.45)),
                            frame="map")
    path = str(tmp_path / "elevation.txt")
    el.save_params(path, p)
    assert el.load_params(path) == p
    with open(path, "a") as f:
        f.write("alpha 3\n")
    with pytest.raises(ValueError):
        el.load_params(path)
    with open(path, "w") as f:
        f.write("# only a comment\nradius 2   # the rest keeps its default\n")
    assert el.load_params(path) == dataclasses.replace(ElevationParams(), radius=2)
    for text in ("height 3\n", "radius\n", "radius two\n", "base_from_cam 1 2 3\n"):
        with open(path, "w") as f:
            f.write(text)
        with pytest.raises(ValueError):
            el.load_params(path)
