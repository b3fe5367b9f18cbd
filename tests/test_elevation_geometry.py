"""The inputs of tests/test_gpu_elevation_geometry.py (tests/golden/elevation_domain.py), judged on the CPU: at every geometry of
postproc_domain.GEOMETRIES and camera step 1, 2 and 4 the vectorised twin equals the plain loop byte for byte, and the inputs do
what they are there for: points are used, every branch of the fusion is taken over the sweep, the second column block of
k_el_scatter and the last column of a 256-column segment carry used points, three mutated readings of the slice walk (the state
forgotten at every launch, the origin or the mount of map k % 64 taken for map k) differ from the twin in the second and in the
third launch, and the big window's known cells lie on both sides of what one pass of k_el_clear covers.  No GPU, no tolerance."""
import numpy as np
import pytest

import elevation_domain as ed
from hobot_stereonet_amd import elevation as el

NAMES = ("trav", "hi", "lo", "rise", "stats")
GEOMS = list(ed.SWEEP)
BRANCHES = ("scrolled", "born", "blended", "up", "down")
_taken = {}           # (w, h, step) -> the branch counts of the twin, for the last test of the sweep


def _q(p, poses):
    return np.stack([el.pose_q(p, x) for x in np.asarray(poses, np.float64).reshape(-1, 3)])


def _differing(a, b):
    return [n for n, x, y in zip(NAMES, a, b) if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes()]


def _twin(w, h, step, raw=None):
    p, cam, poses, maps = ed.case(w, h, step)
    twin = el.Reference(p)
    return twin, twin.push(_q(p, poses), maps if raw is None else raw, cam)


@pytest.mark.parametrize("w,h", GEOMS, ids=[f"{w}x{h}" for w, h in GEOMS])
def test_the_twin_equals_the_plain_loop_at_this_geometry(w, h):
    for step in ed.STEPS:
        p, cam, poses, raw = ed.case(w, h, step)
        assert (p.mw, p.mh, p.cell_m, p.min_points, p.radius) == (21, 18, 0.25, 1, 1) and cam.step == step and raw.shape == (ed.N, h, w)
        twin, a = _twin(w, h, step)
        b = el.LoopReference(p).push(_q(p, poses), raw, cam)
        assert not _differing(a, b), step
        _taken[(w, h, step)] = {k: sum(f[k] for f in twin.frames) for k in BRANCHES}
        print(f"{w}x{h} step {step}: stats {a[4].tolist()}, verdicts of the last map {np.unique(a[0][-1]).tolist()}")
        if w * h >= 3 and step == 1:
            assert a[4][0, 3] > 0, "no point was used"
        if (w, h) in ed.FULL:
            assert a[4][:, 3].min() > 0, ("a map without a used point", step)
            assert set(np.unique(a[0][-1]).tolist()) == {-1, 0, 100}, step


def test_the_sweep_takes_every_branch_of_the_fusion():
    for w, h in GEOMS:
        for step in ed.STEPS:
            if (w, h, step) not in _taken:
                twin, _ = _twin(w, h, step)
                _taken[(w, h, step)] = {k: sum(f[k] for f in twin.frames) for k in BRANCHES}
    total = {k: sum(t[k] for t in _taken.values()) for k in BRANCHES}
    print(total)
    assert all(v > 0 for v in total.values()), total


def test_the_second_column_block_and_the_last_column_carry_used_points():
    """257 x 5 at step 1 is the one case of the older stages' geometries with Wo > 256: without its columns from 256 on the twin's
    bytes are others.  255 x 3 and 256 x 2: the last lane of a 256-column block, idle and busy."""
    _, _, _, raw = ed.case(257, 5, 1)
    cut = raw.copy()
    cut[:, :, 256:] = 0
    whole, less = _twin(257, 5, 1)[1], _twin(257, 5, 1, cut)[1]
    assert _differing(whole, less) and (less[4][:, 3] < whole[4][:, 3]).any()
    # 300 x 20: the second column block carries used points in both of its row chunks (rows 0..9 and 10..19)
    _, _, _, raw = ed.case(300, 20, 1)
    whole = _twin(300, 20, 1)[1]
    for rows in (slice(0, 10), slice(10, 20)):
        cut = raw.copy()
        cut[:, rows, 256:] = 0
        less = _twin(300, 20, 1, cut)[1]
        assert _differing(whole, less) and (less[4][:, 3] < whole[4][:, 3]).any(), rows
    for w, h in ((255, 3), (256, 2)):
        _, _, _, raw = ed.case(w, h, 1)
        cut = raw.copy()
        cut[:, :, -1] = 0
        whole, less = _twin(w, h, 1)[1], _twin(w, h, 1, cut)[1]
        assert (less[4][:, 3] < whole[4][:, 3]).any(), (w, h)


def _walk_twin(forget=False, origin_of=None, mount_of=None):
    """the twin's reading of the slice walk's first push, or a mutated one: `forget` starts every launch with fresh streams,
    origin_of / mount_of map k to the map whose origin / mount it is given"""
    poses, raw, mounts = ed.walk()
    ids, _ = ed.walk_ids()
    q, _ = ed.walk_q()
    if origin_of:
        q = q.copy()
        q[:, 4:] = q[[origin_of(k) for k in range(ed.BIG)], 4:]
    if mount_of:
        mounts = mounts[[mount_of(k) for k in range(ed.BIG)]]
    twin = el.Reference(ed.WALK, 3)
    parts = []
    for k0, m in zip(range(0, ed.BIG, ed.SLICE), ed.launches(ed.BIG)):
        if forget and k0:
            twin.reset()
        parts.append(twin.push(q[k0:k0 + m], raw[k0:k0 + m], ed.WALK_CAM, mounts[k0:k0 + m], ids[k0:k0 + m]))
    return twin, [np.concatenate(x) for x in zip(*parts)]


def test_the_slice_walk_has_teeth():
    twin, want = _walk_twin()
    whole = el.Reference(ed.WALK, 3).push(ed.walk_q()[0], *ed.walk()[1:2], ed.WALK_CAM, ed.walk()[2], ed.walk_ids()[0])
    assert not _differing(want, whole)                   # slice by slice is the one push
    assert ed.launches(ed.BIG) == [64, 64, 2] and ed.launches(ed.SECOND) == [64, 6]
    # the window moved inside every launch, and on the first map of launches two and three whose stream has a past
    ids, _ = ed.walk_ids()
    moved = [f["prev"] not in (None, f["origin"]) for f in twin.frames]
    per_launch = [sum(moved[k0:k0 + m]) for k0, m in zip(range(0, ed.BIG, ed.SLICE), ed.launches(ed.BIG))]
    total = {k: sum(f[k] for f in twin.frames) for k in BRANCHES}
    print(f"the window moved {per_launch} times in the three launches; branches taken {total}")
    assert all(per_launch) and all(v > 0 for v in total.values())
    for k0 in (ed.SLICE, 2 * ed.SLICE):
        k = next(k for k in range(k0, ed.BIG) if ids[k] in ids[:k0])
        assert moved[k], k
    mounts = ed.walk()[2]
    assert len({m.tobytes() for m in mounts}) == ed.BIG
    mutations = {"the state forgotten at every launch": dict(forget=True),
                 "the origin of map k % 64": dict(origin_of=lambda k: k % ed.SLICE),
                 "the mount of map k % 64": dict(mount_of=lambda k: k % ed.SLICE)}
    for name, kw in mutations.items():
        _, got = _walk_twin(**kw)
        per = [[n for n, g, t in zip(NAMES, got, want) if g[k0:k0 + m].tobytes() != t[k0:k0 + m].tobytes()]
               for k0, m in zip(range(0, ed.BIG, ed.SLICE), ed.launches(ed.BIG))]
        print(f"{name}: differing outputs per launch {per}")
        assert not per[0] and per[1] and per[2], name
        assert "trav" in per[1] + per[2] and "hi" in per[1] and "hi" in per[2] and "stats" in per[1] + per[2], name


def test_the_capped_launch_has_longer_chunks_and_points_in_the_last():
    chunks, rows = ed.cap_chunks()
    assert (chunks, rows) == (31, 17) and (ed.CAP_H + 15) // 16 == 33 and ed.CAP_H - (chunks - 1) * rows == 10
    assert ed.cap_chunks(64, 1, 6) == (4, 16) and ed.cap_chunks(5, 2, 3) == (1, 5)      # the launches of the older tests: never capped
    poses, raw = ed.capped()
    q = _q(ed.BASE, poses)
    twin = el.Reference(ed.BASE)
    whole = twin.push(q, raw, ed.CAP_CAM)
    assert whole[4][:, 3].min() > 0 and sum(f["scrolled"] for f in twin.frames) > 0
    for rows_cut in (slice((chunks - 1) * rows, None), slice(16 * 16, 17 * 16)):      # the last chunk; rows that change their chunk
        cut = raw.copy()
        cut[:, rows_cut] = 0
        assert (el.Reference(ed.BASE).push(q, cut, ed.CAP_CAM)[4][:, 3] < whole[4][:, 3]).all(), rows_cut
    assert not _differing([x[:2] for x in whole], el.LoopReference(ed.BASE).push(q[:2], raw[:2], ed.CAP_CAM))


def test_the_big_window_needs_a_second_pass_of_the_clear():
    p = ed.BIG_WINDOW
    poses, raw = ed.big_window()
    cells = p.mw * p.mh
    assert ed.N * cells > ed.CLEAR_PASS
    twin = el.Reference(p)
    out = twin.push(_q(p, poses), raw, ed.CAM)
    print("stats", out[4].tolist())
    assert out[4][:, 0].min() >= 1000
    known = out[1][-1] != el.UNKNOWN
    row, col = divmod(ed.CLEAR_PASS // ed.N, p.mw)
    ys, xs = np.nonzero(known)
    assert ys.min() < row < ys.max() and xs.min() < col < xs.max()
    # the first cell of the second pass lies in the last map: cells that hold points on both sides of it
    first = ed.CLEAR_PASS - (ed.N - 1) * cells
    cnt = el.accumulate(p, _q(p, poses)[-1], *[a[-1] for a in el.base_points(raw, ed.CAM, np.tile(p.matrix(), (ed.N, 1)))])[0].reshape(-1)
    assert 0 < first < cells and cnt[:first].any() and cnt[first:].any()
    assert twin.frames[1]["scrolled"] + twin.frames[2]["scrolled"] > 0


@pytest.mark.parametrize("mw,mh", ed.LIMITS)
def test_windows_at_the_declared_limit_receive_points(mw, mh):
    p, poses, raw = ed.limit_case(mw, mh)
    assert max(mw, mh) == el.MAX_WINDOW and el.check(p) is None and p.radius == 3
    twin = el.Reference(p)
    out = twin.push(_q(p, poses), raw, ed.LIMIT_CAM)
    print(f"{mw}x{mh}: stats {out[4].tolist()}, scrolled {twin.frames[1]['scrolled']}")
    assert out[4][:, 2].min() >= 10 and twin.frames[1]["scrolled"] > 0 and twin.frames[1]["prev"] != twin.frames[1]["origin"]
    if mw * mh <= 4096:      # the plain loop says the same (its verdict is cheap on a window one cell wide)
        assert not _differing(out, el.LoopReference(p).push(_q(p, poses), raw, ed.LIMIT_CAM))


def test_poses_at_the_far_limit_put_known_cells_into_the_window():
    p = ed.FAR
    poses, raw, ids = ed.far_poses()
    q = _q(p, poses)
    assert q[0, 0] == 1 << 30 and q[0, 1] == -(1 << 30) and q[2, 0] == -(1 << 30) and q[2, 1] == 1 << 30
    cell = 256
    for a, b in ((0, 1), (2, 3)):      # within one cell of the limit, and across a cell boundary between the two frames
        assert 0 < np.abs(np.abs(q[b, :2]) - (1 << 30)).min() and np.abs(np.abs(q[b, :2]) - (1 << 30)).max() <= cell
        assert (q[a, 4:] != q[b, 4:]).all()
    with pytest.raises(ValueError):
        el.pose_q(p, (np.nextafter(poses[0, 0], np.inf), 0.0, 0.0))
    twin = el.Reference(p, 2)
    out = twin.push(q, raw, ed.CAM, stream_of=ids)
    print("stats", out[4].tolist())
    assert out[4][:, 0].min() >= 10 and out[4][:, 2].min() >= 10
    assert not _differing(out, el.LoopReference(p, 2).push(q, raw, ed.CAM, stream_of=ids))
