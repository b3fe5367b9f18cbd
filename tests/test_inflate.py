"""Inflation by the robot's radius without a GPU: the numpy twin (hobot_stereonet_amd/inflate.py) equals a brute-force loop
written from the header, the scene the GPU tests rely on takes every branch of the contract, the library's host table
(sn_inflate_table) agrees with the Python restatement within the one unit two exps may differ by, and both sides refuse the
same parameters."""
import ctypes as C
import dataclasses
import functools
import math

import numpy as np
import pytest

from hobot_stereonet_amd import api, inflate
from hobot_stereonet_amd.inflate import InflateParams

ERR_ARG = -1

PARAM_SETS = [inflate.BOUNDARY_P,
              InflateParams(),
              InflateParams(cell_m=0.05, inscribed_radius_m=0.175, inflation_radius_m=1.6, cost_scaling=3.0),      # R = 32
              InflateParams(cell_m=0.1, inscribed_radius_m=0.0, inflation_radius_m=0.0, cost_scaling=1.0),         # R = 0
              InflateParams(cell_m=0.3, inscribed_radius_m=0.3, inflation_radius_m=0.3, cost_scaling=0.0),         # no fall-off band
              InflateParams(cell_m=0.02, inscribed_radius_m=0.11, inflation_radius_m=1.28, cost_scaling=40.0),     # R = 64, zero well inside
              InflateParams(cell_m=1.0, inscribed_radius_m=2.0, inflation_radius_m=7.0, cost_scaling=0.0)]         # flat band


def _equal(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


@functools.lru_cache(maxsize=None)
def _scene():
    p, occ = inflate.boundary_scene()
    occ.setflags(write=False)
    return p, occ, inflate.reference(occ, p, api.inflate_table(p))


def test_twin_equals_the_loop_on_the_boundary_scene():
    p, occ, want = _scene()
    for flags in (0, inflate.UNKNOWN):
        q = dataclasses.replace(p, flags=flags)
        T = api.inflate_table(q)
        assert _equal(inflate.reference(occ, q, T), inflate.loop_reference(occ, q, T)), flags


def test_every_branch_of_the_boundary_scene_is_taken():
    p, occ, want = _scene()
    br = want[4]
    print(br)
    assert set(br) == set(inflate.BRANCHES)
    for name in inflate.BRANCHES:
        assert br[name] > 0, name
    assert inflate.radius_cells(p) == 4 and api.inflate_table(p)[16] == 0 and api.inflate_table(p)[15] > 0
    # the flag decides the cells of the third regime, and nothing else
    flagged = inflate.reference(occ, dataclasses.replace(p, flags=inflate.UNKNOWN), api.inflate_table(p))
    assert int((flagged[0] != want[0]).sum()) == br["unknown_flag_only"]
    # map 2 has no obstacle: nothing but 0 and 255, nothing reached
    assert set(np.unique(want[0][2])) == {0, 255} and np.all(want[2][2] == inflate.NOT_REACHED)


@pytest.mark.parametrize("R", [0, 1, 3, 7])
def test_twin_equals_the_loop_on_random_grids(R):
    rng = np.random.default_rng(100 + R)
    for gw, gh, density in ((40, 24, 0.01), (17, 9, 0.05), (1, 1, 0.15), (1, 13, 0.1), (23, 1, 0.1), (9, 30, 0.002)):
        p = InflateParams(cell_m=0.125, inscribed_radius_m=0.125 * min(R, 1.5), inflation_radius_m=0.125 * R, cost_scaling=2.5, lethal_min=70,
                          flags=R & 1)
        assert inflate.radius_cells(p) == R
        occ = rng.choice(np.array([-1, 0, 69, 70, 100], np.int8), (2, gh, gw), p=(0.4, 0.6 - 3 * density, density, density, density))
        a, b = inflate.reference(occ, p), inflate.loop_reference(occ, p)
        assert _equal(a, b), (gw, gh)
        assert np.array_equal(a[3].sum(1), [gw * gh] * 2)                        # the stats sum to the grid
        assert np.array_equal(a[1], inflate.translate(a[0]))


def test_library_table_against_the_python_restatement():
    for p in PARAM_SETS:
        T, mine = api.inflate_table(p), inflate.table(p)
        R = inflate.radius_cells(p)
        assert T.shape == mine.shape == (R * R + 1,), p
        assert np.abs(T.astype(int) - mine.astype(int)).max() <= 1, p
        assert T[0] == 254 and np.all(np.diff(T.astype(int)) <= 0), p            # non-increasing
        if p.cost_scaling == 0.0:
            assert np.array_equal(T, mine), p                                    # exp(-0) = 1 on both sides
    flat = api.inflate_table(PARAM_SETS[-1])
    assert set(flat[5:50]) == {252} and flat[4] == 253 and flat[49] == 252      # dist 2 inscribed; the band at 252 up to dist 7
    assert np.any(api.inflate_table(PARAM_SETS[5])[: 64 * 64] == 0)


def test_radius_of_64_cells_is_accepted_and_65_refused():
    ok = InflateParams(cell_m=0.05, inscribed_radius_m=0.1, inflation_radius_m=3.2, cost_scaling=1.0)
    assert inflate.radius_cells(ok) == 64 and inflate.check(ok) is None and api.inflate_table(ok).shape == (4097,)
    for infl in (3.2001, 3.25, 100.0):
        bad = dataclasses.replace(ok, inflation_radius_m=infl)
        assert inflate.radius_cells(bad) >= 65 and inflate.check(bad) == "the inflation radius must be at most 64 cells"
        with pytest.raises(api.StereoNetError):
            api.inflate_table(bad)


def test_check_and_the_library_refuse_the_same_parameters():
    lib = api.load_library()
    good = inflate.BOUNDARY_P
    cases = [dict(), dict(flags=1), dict(lethal_min=1), dict(lethal_min=100), dict(inscribed_radius_m=0.0), dict(cost_scaling=0.0),
             dict(inscribed_radius_m=1.0), dict(cell_m=1e-30, inflation_radius_m=0.0, inscribed_radius_m=0.0),
             dict(cell_m=0.0), dict(cell_m=-0.25), dict(cell_m=math.nan), dict(cell_m=math.inf), dict(inscribed_radius_m=-0.1),
             dict(inscribed_radius_m=math.nan), dict(inflation_radius_m=0.2), dict(inflation_radius_m=math.inf),
             dict(inflation_radius_m=math.nan), dict(cost_scaling=-1.0), dict(cost_scaling=math.inf), dict(cost_scaling=math.nan),
             dict(inflation_radius_m=16.3), dict(cell_m=1e-30), dict(lethal_min=0), dict(lethal_min=101), dict(lethal_min=-5),
             dict(flags=2), dict(flags=3), dict(flags=-1)]
    refused = 0
    for kw in cases:
        p = dataclasses.replace(good, **kw)
        why = inflate.check(p)
        c_p, R = api.inflate_params(p), C.c_int(-7)
        rc = lib.sn_inflate_table(C.byref(c_p), None, C.byref(R))
        assert (rc == ERR_ARG) == (why is not None) and rc in (0, ERR_ARG), (kw, why, rc)
        assert (R.value == -7) == (why is not None), kw                           # a refusal writes nothing
        refused += why is not None
    assert refused == 20
    assert lib.sn_inflate_table(None, None, None) == ERR_ARG
    c_p = api.inflate_params(good)
    assert lib.sn_inflate_table(C.byref(c_p), None, None) == 0                    # both outputs are optional


def test_translate():
    got = inflate.translate(np.array([0, 1, 252, 253, 254, 255, 2, 127], np.uint8))
    assert got.dtype == np.int8 and got.tolist() == [0, 1, 98, 99, 100, -1, 1, 49]
    assert np.all(np.diff(inflate.translate(np.arange(255, dtype=np.uint8)).astype(int)) >= 0)


def test_stats_sum_to_the_grid():
    p, occ, want = _scene()
    assert np.array_equal(want[3].sum(1), [occ.shape[1] * occ.shape[2]] * occ.shape[0])
    assert want[3][2].tolist()[:3] == [0, 0, 0]


def test_parameter_file_round_trip(tmp_path):
    path = str(tmp_path / "inflate.txt")
    for p in PARAM_SETS + [InflateParams(cell_m=0.1 + 1e-9, cost_scaling=1 / 3, lethal_min=77, flags=1)]:
        inflate.save_params(path, p)
        assert inflate.load_params(path) == p
    (tmp_path / "part.txt").write_text("# only one key\nlethal_min 80   # the rest keep their defaults\n")
    assert inflate.load_params(str(tmp_path / "part.txt")) == InflateParams(lethal_min=80)
    for text in ("radius 3\n", "lethal_min 1\nlethal_min 2\n", "cell_m 0.1 0.2\n", "cell_m abc\n", "lethal_min 1.5\n"):
        (tmp_path / "bad.txt").write_text(text)
        with pytest.raises(ValueError):
            inflate.load_params(str(tmp_path / "bad.txt"))
