"""The navigation function without a GPU: the heapq twin (hobot_stereonet_amd/navfn.py) equals a plain relaxation loop written
from the header, the field satisfies the contract's inequalities with equality somewhere at every finite cell, the path's cost is
P(start), it cuts no corner and follows the stated tie order, uint32 holds the worst route, every flag has its case, and the
parameter file round-trips."""
import dataclasses
import functools

import numpy as np
import pytest

from hobot_stereonet_amd import navfn
from hobot_stereonet_amd.navfn import INF, MOVES, NavParams


def _random_cost(rng, n, gh, gw):
    """the full byte range, with enough free cells that the goal's component is more than a few cells"""
    c = rng.integers(0, 256, (n, gh, gw)).astype(np.uint8)
    c[rng.random((n, gh, gw)) < 0.45] = 0
    return c


@pytest.mark.parametrize("flags,lethal", [(0, 253), (1, 253), (0, 100), (1, 100)])
def test_twin_equals_the_plain_relaxation_loop(flags, lethal):
    rng = np.random.default_rng(7 + flags + lethal)
    reached = 0
    for gw, gh in ((12, 9), (9, 12), (1, 1), (1, 7), (8, 1), (5, 5)):
        p = NavParams(neutral=int(rng.integers(1, 256)), lethal_cost=lethal, unknown_cost=int(rng.integers(0, 253)), flags=flags)
        cost = _random_cost(rng, 4, gh, gw)
        goals = np.stack([rng.integers(0, gw, 4), rng.integers(0, gh, 4)], 1)
        cost[0, goals[0, 1], goals[0, 0]] = 0                     # a passable goal in map 0 whatever the draw
        pot, path, stats = navfn.reference(cost, goals, None, p)
        assert path is None and pot.dtype == np.uint32 and stats.dtype == np.uint32
        for k in range(4):
            loop = navfn.loop_relaxation(cost[k], goals[k], p)
            assert pot[k].tobytes() == loop.tobytes(), (gw, gh, k)
            assert stats[k, 1] == (loop != INF).sum() and stats[k, 4] == (navfn.weights(cost[k], p) == 0).sum()
        reached += int(stats[:, 1].sum())
    assert reached > 100


@functools.lru_cache(maxsize=None)
def _large(flags):
    """three seeded maps of 150 x 40 with walls, and the twin's answer: shared by the tests and never changed"""
    rng = np.random.default_rng(31 + flags)
    gw, gh = 150, 40
    cost = rng.choice(np.array([0, 30, 120, 252, 253, 254, 255], np.uint8), (3, gh, gw), p=(0.55, 0.1, 0.1, 0.07, 0.04, 0.04, 0.1))
    cost[:, :, 40], cost[:, :, 90] = 254, 254
    cost[:, 4:7, 39:42], cost[:, 32:35, 89:92] = 0, 0              # one gap per wall, three cells tall
    goals = np.array([[140, 35], [3, 3], [75, 20]])
    starts = np.array([[2, 2], [149, 39], [10, 30]])
    for k in range(3):
        for x, y in (goals[k], starts[k]):
            cost[k, y - 1:y + 2, x - 1:x + 2] = 0
    p = NavParams(neutral=50, lethal_cost=253, unknown_cost=17, flags=flags, max_path=2000)
    out = navfn.reference(cost, goals, starts, p)
    for a in (cost,) + out:
        a.setflags(write=False)
    return p, cost, goals, starts, out


@pytest.mark.parametrize("flags", [0, 1])
def test_the_field_satisfies_the_contract_on_larger_grids(flags):
    p, cost, goals, starts, (pot, path, stats) = _large(flags)
    n, gh, gw = cost.shape
    W = navfn.weights(cost, p)
    P = pot.astype(np.int64)
    P[pot == INF] = 1 << 62
    pad_w = np.pad(W, ((0, 0), (1, 1), (1, 1)))
    pad_p = np.pad(P, ((0, 0), (1, 1), (1, 1)), constant_values=1 << 62)
    best = np.full(P.shape, 1 << 62, np.int64)
    for d, (dx, dy) in enumerate(MOVES):
        wa = pad_w[:, 1 + dy:1 + dy + gh, 1 + dx:1 + dx + gw]
        pa = pad_p[:, 1 + dy:1 + dy + gh, 1 + dx:1 + dx + gw]
        ok = (W > 0) & (wa > 0)
        if d & 1:
            ok &= (pad_w[:, 1:1 + gh, 1 + dx:1 + dx + gw] > 0) & (pad_w[:, 1 + dy:1 + dy + gh, 1:1 + gw] > 0)
        cand = np.where(ok & (pa < 1 << 62), pa + (7 if d & 1 else 5) * W, 1 << 62)
        assert np.all(P <= cand)                                   # P(b) <= P(a) + k w(b) for every allowed move
        best = np.minimum(best, cand)
    finite = pot != INF
    goal = np.zeros_like(finite)
    goal[np.arange(n), goals[:, 1], goals[:, 0]] = True
    assert np.all(pot[goal] == 0) and np.all(P[finite & ~goal] == best[finite & ~goal])      # ... with equality somewhere
    assert np.all(best[~finite & (W > 0)] == 1 << 62) and not np.any(finite & (W == 0))
    assert np.all(stats[:, 0] == 0) and np.all(stats[:, 1] > 1500)


@pytest.mark.parametrize("flags", [0, 1])
def test_the_path_costs_p_start_and_cuts_no_corner(flags):
    p, cost, goals, starts, (pot, path, stats) = _large(flags)
    W = navfn.weights(cost, p)
    for k in range(cost.shape[0]):
        length = int(stats[k, 2])
        cells = [tuple(int(v) for v in c) for c in path[k, :length]]
        assert 50 < length <= p.max_path and np.all(path[k, length:] == -1)
        assert cells[0] == tuple(starts[k]) and cells[-1] == tuple(goals[k]) and len(set(cells)) == length
        assert navfn.path_cost(cells, cost[k], p) == stats[k, 3] == pot[k, starts[k, 1], starts[k, 0]]
        for (x, y), (ax, ay) in zip(cells[:-1], cells[1:]):
            assert max(abs(ax - x), abs(ay - y)) == 1 and W[k, y, x] > 0 and W[k, ay, ax] > 0
            assert W[k, y, ax] > 0 and W[k, ay, x] > 0             # the squeezed cells (the ends themselves on a straight move)
            assert pot[k, ay, ax] < pot[k, y, x]


def test_ties_follow_the_stated_order_on_a_uniform_grid():
    p = NavParams(neutral=10, max_path=64)
    cost = np.zeros((1, 9, 9), np.uint8)
    goal = (4, 4)
    # the first move out of (x, y): the contract's order is E, NE, N, NW, W, SW, S, SE, lowest index first
    first = {}
    for sx in range(9):
        for sy in range(9):
            if (sx, sy) == goal:
                continue
            pot, path, stats = navfn.reference(cost, [goal], [(sx, sy)], p)
            cells = path[0, :stats[0, 2]]
            step = (int(cells[1, 0]) - sx, int(cells[1, 1]) - sy)
            # every neighbour that ties for the minimum, by hand: P on a uniform grid is 50 * straight + 70 * diagonal moves
            keys = []
            for d, (dx, dy) in enumerate(MOVES):
                ax, ay = sx + dx, sy + dy
                if 0 <= ax < 9 and 0 <= ay < 9:
                    far = (abs(ax - 4), abs(ay - 4))
                    keys.append((70 * min(far) + 50 * (max(far) - min(far)) + (70 if d & 1 else 50), d))
            assert step == MOVES[min(keys)[1]], (sx, sy)
            first[(sx, sy)] = navfn.MOVE_NAMES[MOVES.index(step)]
            assert navfn.path_cost([tuple(c) for c in cells], cost[0], p) == stats[0, 3]
    # a knight's move away two routes tie: NE then N, or N then NE, and so on round the compass: the lower index goes first
    assert first[(3, 6)] == "NE" and first[(5, 6)] == "N" and first[(2, 3)] == "E" and first[(2, 5)] == "E" and first[(6, 5)] == "NW"
    assert first[(6, 3)] == "W" and first[(3, 2)] == "S" and first[(5, 2)] == "SW"


def test_uint32_holds_the_worst_route():
    """a serpentine of the heaviest passable cells: the route visits every free cell, nearly all of it in diagonal-free straight
    moves at 5 * 509; scaled to 2^20 cells at 7 * 509 a cell, the header's bound, it stays below 2^32 - 1"""
    p = NavParams(neutral=255, lethal_cost=255, max_path=400)
    gw, gh = 9, 9
    cost = np.full((gh, gw), 255, np.uint8)                       # blocked (no flag)
    for y in range(0, gh, 2):
        cost[y, :] = 254                                          # corridors of the heaviest passable cell: w = 509
    for i, y in enumerate(range(1, gh, 2)):
        cost[y, gw - 1 if i % 2 == 0 else 0] = 254                # joined at alternating ends
    free = int((navfn.weights(cost, p) > 0).sum())
    pot, path, stats = navfn.reference(cost, [(gw - 1, gh - 1)], [(0, 0)], p)
    assert stats[0, 2] == free == stats[0, 1]                     # the path visits every passable cell
    assert stats[0, 3] == 5 * 509 * (free - 1) <= navfn.worst_potential(free)
    assert int(pot[pot != INF].max()) == stats[0, 3]
    assert navfn.worst_potential(navfn.MAX_AREA) == 3736072725 < INF and navfn.worst_potential(navfn.MAX_AREA) + 7 * 509 < INF
    with pytest.raises(ValueError):
        navfn.reference(np.zeros((1025, 1024), np.uint8), [(0, 0)], None, p)


def test_flags_one_case_each():
    p = NavParams(neutral=1, max_path=8)
    cost = np.zeros((4, 6), np.uint8)
    cost[:, 3] = 254
    ok = navfn.reference(cost, [(0, 0)], [(2, 3)], p)[2][0]
    assert ok.tolist() == [0, 12, 4, 7 + 7 + 5, 4]
    for goal in ((3, 1), (-1, 0), (6, 0), (0, 4)):                # blocked, and outside on three sides
        pot, path, st = navfn.reference(cost, [goal], [(2, 3)], p)
        assert st[0].tolist() == [navfn.GOAL_BLOCKED | navfn.START_UNREACHABLE, 0, 0, INF, 4] and np.all(pot == INF) and np.all(path == -1)
    assert navfn.reference(cost, [(3, 1)], None, p)[2][0].tolist() == [navfn.GOAL_BLOCKED, 0, 0, INF, 4]
    for start in ((3, 0), (5, 2), (0, -1), (6, 6)):               # blocked, behind the wall, outside
        st = navfn.reference(cost, [(0, 0)], [start], p)[2][0]
        assert st.tolist() == [navfn.START_UNREACHABLE, 12, 0, INF, 4], start
    pot, path, st = navfn.reference(cost, [(0, 0)], [(2, 3)], dataclasses.replace(p, max_path=3))
    assert st[0].tolist() == [navfn.PATH_TRUNCATED, 12, 4, 19, 4] and path[0].tolist() == [[2, 3], [2, 2], [1, 1]]
    pot, path, st = navfn.reference(cost, [(0, 0)], [(2, 3)], dataclasses.replace(p, max_path=4))
    assert st[0, 0] == 0 and path[0, 3].tolist() == [0, 0]
    assert navfn.reference(cost, [(0, 0)], [(0, 0)], p)[2][0].tolist() == [0, 12, 1, 0, 4]      # start = goal: a path of one cell
    # unknown cells: blocked without the flag, priced with it, and 255 is tested before lethal_cost
    cost[:, 3] = 255
    assert navfn.reference(cost, [(0, 0)], [(5, 0)], p)[2][0, 0] == navfn.START_UNREACHABLE
    st = navfn.reference(cost, [(0, 0)], [(5, 0)], NavParams(neutral=1, unknown_cost=9, flags=navfn.UNKNOWN_OK, max_path=8))[2][0]
    assert st.tolist() == [0, 24, 6, 5 * (1 + 1 + 10 + 1 + 1), 0]
    st = navfn.reference(cost, [(0, 0)], [(5, 0)], NavParams(neutral=1, lethal_cost=1, unknown_cost=9, flags=navfn.UNKNOWN_OK))[2][0]
    assert st[0] == 0 and st[4] == 0
    for bad in (dict(neutral=0), dict(neutral=256), dict(lethal_cost=0), dict(lethal_cost=256), dict(unknown_cost=253), dict(unknown_cost=-1),
                dict(flags=2), dict(max_rounds=-1), dict(max_path=-1)):
        assert navfn.check(dataclasses.replace(p, **bad)) is not None, bad
    assert navfn.check(NavParams(neutral=255, lethal_cost=255, unknown_cost=252, flags=1, max_rounds=0, max_path=0)) is None


def test_a_diagonal_pinch_is_not_squeezed_through():
    p = NavParams(neutral=1, max_path=16)
    cost = np.zeros((4, 4), np.uint8)
    cost[1, 2] = cost[2, 1] = 254                                 # (1, 1) and (2, 2) touch at a corner between two blocked cells
    pot, path, st = navfn.reference(cost, [(3, 3)], [(0, 0)], p)
    cells = [tuple(c) for c in path[0, :st[0, 2]].tolist()]
    assert (1, 1) not in cells[1:] or (2, 2) not in cells         # never one after the other
    assert st[0, 3] == navfn.path_cost(cells, cost, p) and st[0, 3] > 3 * 7
    cost[1, 2] = 0                                                # one of the two gone: the diagonal is still closed
    assert navfn.reference(cost, [(2, 2)], [(1, 1)], p)[2][0, 3] == 10


def test_parameter_file_round_trip(tmp_path):
    path = str(tmp_path / "plan.txt")
    for p in (NavParams(), NavParams(neutral=1, lethal_cost=100, unknown_cost=252, flags=1, max_rounds=40, max_path=7, goal=(399, 0), start=(-3, 12)),
              NavParams(goal=(5, 6))):
        navfn.save_params(path, p)
        assert navfn.load_params(path) == p
    (tmp_path / "part.txt").write_text("# only two keys\ngoal 7 8   # the rest keep their defaults\nneutral 66\n")
    assert navfn.load_params(str(tmp_path / "part.txt")) == NavParams(neutral=66, goal=(7, 8))
    for text in ("radius 3\n", "neutral 1\nneutral 2\n", "goal 1\n", "goal 1 2 3\n", "neutral abc\n", "neutral 1.5\n", "start 1 2\nstart 1 2\n"):
        (tmp_path / "bad.txt").write_text(text)
        with pytest.raises(ValueError):
            navfn.load_params(str(tmp_path / "bad.txt"))


def test_constants_are_the_headers():
    import os
    import re
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "stereonet_hip.h")).read()
    defs = {k: v for k, v in re.findall(r"#define\s+(SN_NAV_\w+)\s+(\(1 << 20\)|0x[0-9A-Fa-f]+u?|\d+)", text)}
    value = lambda k: (1 << 20) if defs[k].startswith("(") else int(defs[k].rstrip("u"), 0)      # noqa: E731
    assert (value("SN_NAV_TILE_W"), value("SN_NAV_TILE_H")) == (navfn.TILE_W, navfn.TILE_H)
    assert value("SN_NAV_MAX_CELLS") == navfn.MAX_AREA and value("SN_NAV_INF") == INF and value("SN_NAV_UNKNOWN_OK") == navfn.UNKNOWN_OK
    assert [value(k) for k in ("SN_NAV_GOAL_BLOCKED", "SN_NAV_START_UNREACHABLE", "SN_NAV_PATH_TRUNCATED", "SN_NAV_UNCONVERGED")] == \
        [navfn.GOAL_BLOCKED, navfn.START_UNREACHABLE, navfn.PATH_TRUNCATED, navfn.UNCONVERGED]


def test_the_scaled_picture():
    pot = np.array([[0, 10, 20], [INF, 5, 20]], np.uint32)
    assert navfn.scale_potential(pot).tolist() == [[0, 127, 254], [255, 63, 254]]
    assert navfn.scale_potential(np.full((2, 2), INF, np.uint32)).tolist() == [[255, 255], [255, 255]]
