"""The left-right consistency check as its numpy twin (hobot_stereonet_amd/lrcheck.py) — no GPU.  Analytic occlusion scenes
(everything the right eye cannot see is rejected, and little else), mirrored storage, reason priority and corner values against
a per-pixel scalar transcription of the contract in include/stereonet_hip.h (tests/golden/plain_refs.py), the eye-swapping mirror, and the agreement of the
Python binding with the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hobot_stereonet_amd import api, lrcheck
from hobot_stereonet_amd.lrcheck import INCONSISTENT, INVALID_IN, KEPT, NO_PARTNER, OUT_OF_VIEW
from plain_refs import lrcheck_scalar as _scalar_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "stereonet_hip.h")).read()
S = lrcheck.wire_scale()
f32 = np.float32


def _to_raw(d):
    return np.rint(np.asarray(d, np.float64) / np.float64(S)).astype(np.int32)


# (W, d0, d1, a, b) -> occluded pixels, out-of-view pixels, further rejected columns per row
SCENES = [((96, 8.0, 20.0, 40, 60), 12, 8, set()),
          ((96, 8.5, 20.25, 40, 60), 11, 9, {28, 40}),
          ((1280, 31.3, 97.7, 500, 800), 66, 32, {500}),
          ((1242, 12.25, 200.6, 601, 777), 176, 13, {589, 601})]


def _scene(W, d0, d1, a, b, rows=3):
    x = np.arange(W, dtype=np.float64)
    dl = np.where((x >= a) & (x < b), d1, d0)
    dr = np.where((x >= a - d1) & (x < b - d1), d1, d0)
    occluded = (x < a) & (x - d0 >= a - d1) & (x - d0 < b - d1)
    out_of_view = x - dl < 0
    rep = lambda m: np.repeat(m[None], rows, 0)      # noqa: E731
    return rep(_to_raw(dl)), rep(_to_raw(dr)), occluded, out_of_view


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("scene,n_occ,n_oov,extra_cols", SCENES)
def test_analytic_occlusion_scenes(scene, n_occ, n_oov, extra_cols, mirrored):
    W, d0, d1, a, b = scene
    rl, rr, occluded, oov = _scene(*scene)
    assert int(occluded.sum()) == n_occ and int(oov.sum()) == n_oov          # the scene is the one the figures belong to
    out, mask, kept = lrcheck.reference(rl, rr[..., ::-1] if mirrored else rr, 1.0, 0.0, mirrored)
    occ_cols = np.flatnonzero(occluded)
    near = {occ_cols[0] - 1, occ_cols[0], occ_cols[0] + 1, occ_cols[-1] - 1, occ_cols[-1], occ_cols[-1] + 1, a - 1, a, a + 1}
    for row in mask:
        assert np.all(row[oov] == OUT_OF_VIEW)                                 # (a)
        assert np.all(row[occluded] != KEPT)                                   # (b)
        extra = set(np.flatnonzero((row != KEPT) & ~occluded & ~oov).tolist())
        print(scene, "mirrored" if mirrored else "plain", "further rejected columns:", sorted(extra))
        assert len(extra) <= 3 and extra <= near                               # (c): a condition, not a tolerance
        assert extra == extra_cols
    assert np.array_equal(out, np.where(mask == KEPT, rl, 0))
    assert kept.tolist() == [(W - n_occ - n_oov - len(extra_cols)) * 3]


def _random_maps(rng, n, h, w, dmax):
    """maps around a common smooth surface (so that many pixels are consistent), ~30 % holes, corner values"""
    base = rng.uniform(1.0, dmax, (n, h, 1)) + np.cumsum(rng.normal(0, 0.4, (n, h, w)), -1)
    l = _to_raw(np.clip(base + rng.normal(0, 0.6, base.shape), 0.01, None))
    r = _to_raw(np.clip(base + rng.normal(0, 0.6, base.shape), 0.01, None))
    for m in (l, r):
        m[rng.random(m.shape) < 0.3] = 0
        m[rng.random(m.shape) < 0.02] = -7
    l[0, 0, :4] = [-7, 0, 1, 2 ** 31 - 1]
    l[-1, -1, -2:] = [1, 2 ** 31 - 1]
    return l, r


def test_mirrored_storage_equals_plain_storage_and_the_scalar_contract():
    rng = np.random.default_rng(5)
    for w, taus in ((37, (1.0, 0.0)), (64, (0.5, 0.02)), (50, (0.0, 0.0))):
        l, r = _random_maps(rng, 2, 5, w, 20.0)
        plain = lrcheck.reference(l, r, *taus, mirrored=False)
        mirr = lrcheck.reference(l, np.ascontiguousarray(r[..., ::-1]), *taus, mirrored=True)
        for p, m in zip(plain, mirr):
            assert np.array_equal(p, m)
        assert len(set(np.unique(plain[1]).tolist())) >= 4                    # the maps exercise the reasons
        for k in range(2):
            for mirrored, got in ((False, plain), (True, mirr)):
                want = _scalar_reference(l[k], r[k][..., ::-1] if mirrored else r[k], *taus, mirrored)
                assert np.array_equal(got[0][k], want[0]) and np.array_equal(got[1][k], want[1]) and got[2][k] == want[2]
        single = lrcheck.reference(l[0], r[0], *taus)
        assert np.array_equal(single[0], plain[0][0]) and np.array_equal(single[1], plain[1][0]) and single[2][0] == plain[2][0]


def test_reason_priority_and_corner_values():
    W = 8
    r10 = int(_to_raw(2.0))                     # 2 px
    # raw_left corner values; the right map is valid everywhere unless a case says otherwise
    L = np.array([[-7, 0, 1, 2 ** 31 - 1, r10, r10, r10, 1]], np.int32)
    R = np.full((1, W), r10, np.int32)
    R[0, 7] = 1                                 # agrees with the left map's raw = 1 at u = 7 only through the interpolation
    out, mask, kept = lrcheck.reference(L, R, 1.0, 0.0)
    #  u=0: -7 -> INVALID_IN; u=1: 0 -> INVALID_IN; u=2: raw 1, d = 5e-4: partner R(1), R(2) = 2 px -> |d - dr| ~ 2 > 1;
    #  u=3: 2^31-1 -> d ~ 1.07e6 px -> OUT_OF_VIEW; u=4..6: d = 2 -> partner 2 px -> kept;
    #  u=7 = W-1 with d < 1: x0 = 6, x1 = 7 (= W-1), t = 0.9995: dr = 2 + t*(5e-4 - 2) ~ 1.5e-3 -> kept
    assert mask[0].tolist() == [INVALID_IN, INVALID_IN, INCONSISTENT, OUT_OF_VIEW, KEPT, KEPT, KEPT, KEPT]
    assert out[0].tolist() == [0, 0, 0, 0, r10, r10, r10, 1] and kept.tolist() == [4]
    # INVALID_IN wins over everything, OUT_OF_VIEW over NO_PARTNER: an empty right map
    _, m0, k0 = lrcheck.reference(L, np.zeros_like(R), 1.0, 0.0)
    assert m0[0].tolist() == [INVALID_IN, INVALID_IN, NO_PARTNER, OUT_OF_VIEW] + [NO_PARTNER] * 4 and k0.tolist() == [0]
    # a partner with one sample <= 0 takes the other sample's disparity; with both <= 0 there is no partner
    L2 = np.zeros((1, W), np.int32)
    L2[0, 5] = int(_to_raw(2.5))                # xr = 2.5: samples R(2), R(3)
    for r2, r3, want in ((0, L2[0, 5], KEPT), (L2[0, 5], -3, KEPT), (0, -3, NO_PARTNER), (int(_to_raw(9.0)), 0, INCONSISTENT),
                         (int(_to_raw(1.0)), int(_to_raw(4.0)), KEPT), (int(_to_raw(1.0)), int(_to_raw(7.0)), INCONSISTENT)):
        R2 = np.full((1, W), 123456, np.int32)
        R2[0, 2], R2[0, 3] = r2, r3
        assert lrcheck.reference(L2, R2, 1.0, 0.0)[1][0, 5] == want, (r2, r3)
        assert lrcheck.reference(L2, R2[..., ::-1], 1.0, 0.0, mirrored=True)[1][0, 5] == want, (r2, r3)
    # only the relative term lets the pixel pass: d = 100 px against dr = 103 px
    Wb = 256
    L3 = np.zeros((1, Wb), np.int32)
    R3 = np.zeros((1, Wb), np.int32)
    L3[0, 200] = int(_to_raw(100.0))
    R3[0, 99:102] = int(_to_raw(103.0))
    assert lrcheck.reference(L3, R3, 1.0, 0.0)[1][0, 200] == INCONSISTENT
    assert lrcheck.reference(L3, R3, 1.0, 0.05)[1][0, 200] == KEPT            # 3 <= 1 + 0.05 * 100
    assert lrcheck.reference(L3, R3, 1.0, 0.019)[1][0, 200] == INCONSISTENT   # 3 >  1 + 0.019 * 100
    # tau = 0: only exact agreement survives
    L4 = np.full((1, W), r10, np.int32)
    at2 = OUT_OF_VIEW if f32(2) - f32(r10) * S < 0 else KEPT                  # the quantised 2 px may sit on either side of 2
    assert lrcheck.reference(L4, L4, 0.0, 0.0)[1][0].tolist() == [OUT_OF_VIEW] * 2 + [at2] + [KEPT] * 5
    # where x1 really clamps: (float)(W-1) - d rounds back to W-1 once W-1 >= 2^14 (d = 5e-4 is below half an ulp there)
    Wc = 2 ** 14 + 2
    L5 = np.zeros((1, Wc), np.int32)
    R5 = np.zeros((1, Wc), np.int32)
    L5[0, -1], R5[0, -1] = 1, 1
    assert f32(Wc - 1) - f32(1) * S == f32(Wc - 1)
    assert lrcheck.reference(L5, R5, 0.0, 0.0)[1][0, -1] == KEPT
    assert _scalar_reference(L5, R5, 0.0, 0.0, False)[1][0, -1] == KEPT
    for bad in ((-1.0, 0.0), (0.0, -0.5), (float("nan"), 0.0), (1.0, float("inf"))):
        with pytest.raises(ValueError):
            lrcheck.reference(L, R, *bad)



def _contraction_sensitive_maps(w):
    """One pixel per row whose outcome changes if u - rl*S is evaluated as ONE fused multiply-add: (float)rl * S rounds to the
    integer m while the exact product lies above m by more than an ulp of the small number k.  Rounded separately, xr = u - m = k exactly (t = 0: the partner is R(k)
    alone, which agrees -> kept at tau = 0); fused, xr falls just below k (x0 = k - 1, t ~ 1: the disagreeing neighbour leaks in
    -> inconsistent).  -> (left, right, columns)"""
    s32 = lrcheck.wire_scale()
    cand = np.arange(int(64 / float(s32)), int((w - 80) / float(s32)), dtype=np.int64)
    p32 = cand.astype(np.float32) * s32
    exact = cand.astype(np.float64) * np.float64(s32)                  # 24 x 24 bits: exact in double
    rl = cand[(p32 == np.rint(p32)) & (exact - p32.astype(np.float64) > 8e-6)][:96]      # ulp(k) <= 3.8e-6 for k < 64
    assert len(rl) >= 16
    m = np.rint(rl.astype(np.float32) * s32).astype(np.int64)
    k = 5 + np.arange(len(rl)) % 50
    left = np.zeros((len(rl), w), np.int32)
    right = np.full((len(rl), w), 77, np.int32)
    rows = np.arange(len(rl))
    left[rows, m + k] = rl
    right[rows, k - 1] = rl + 6000
    right[rows, k] = rl
    right[rows, k + 1] = rl + 6000
    fused_xr = ((m + k).astype(np.float64) - rl.astype(np.float64) * np.float64(s32)).astype(np.float32)
    assert np.all(np.floor(fused_xr) == k - 1)                         # what a contracted kernel would compute
    return left, right, m + k


def test_every_operation_is_rounded_on_its_own():
    """The twin is the unfused evaluation: on pixels built so that a fused u - rl*S lands in the column before, it keeps them."""
    left, right, cols = _contraction_sensitive_maps(1280)
    rows = np.arange(len(cols))
    for mirrored in (False, True):
        out, mask, kept = lrcheck.reference(left, right[..., ::-1] if mirrored else right, 0.0, 0.0, mirrored)
        assert np.all(mask[rows, cols] == KEPT) and kept.tolist() == [len(cols)]
    want = _scalar_reference(left[:8], right[:8], 0.0, 0.0, False)
    assert np.array_equal(lrcheck.reference(left[:8], right[:8], 0.0, 0.0)[1], want[1])


def test_mirror_pair_is_an_involution_and_matches_the_formula():
    rng = np.random.default_rng(2)
    for shape in ((6, 5, 7), (3, 6, 4, 16), (2, 6, 3, 1242)):
        x = rng.integers(-128, 128, shape, dtype=np.int8)
        y = lrcheck.mirror_pair(x)
        assert y.shape == x.shape and y.dtype == np.int8 and y.flags.c_contiguous
        assert np.array_equal(lrcheck.mirror_pair(y), x)
        x4, y4 = x.reshape((-1,) + x.shape[-3:]), y.reshape((-1,) + x.shape[-3:])
        W = x.shape[-1]
        for k in range(x4.shape[0]):
            for c in range(6):
                for u in (0, 1, W // 2, W - 1):
                    assert np.array_equal(y4[k, c, :, u], x4[k, (c + 3) % 6, :, W - 1 - u])
    with pytest.raises(ValueError):
        lrcheck.mirror_pair(np.zeros((5, 4, 4), np.int8))


def test_binding_agrees_with_the_header():
    enums = {k: int(v) for k, v in re.findall(r"\b(SN_LRC_[A-Z0-9_]+)\s*=\s*(\d+)", HEADER)}
    assert set(enums) == {"SN_LRC_KEPT", "SN_LRC_INVALID_IN", "SN_LRC_OUT_OF_VIEW", "SN_LRC_NO_PARTNER", "SN_LRC_INCONSISTENT",
                          "SN_LRC_IN_TENSOR", "SN_LRC_IN_SBS_NV12"}
    for name, value in enums.items():
        assert getattr(api, name) == value, name
    assert (lrcheck.KEPT, lrcheck.INVALID_IN, lrcheck.OUT_OF_VIEW, lrcheck.NO_PARTNER, lrcheck.INCONSISTENT) == tuple(
        enums[k] for k in ("SN_LRC_KEPT", "SN_LRC_INVALID_IN", "SN_LRC_OUT_OF_VIEW", "SN_LRC_NO_PARTNER", "SN_LRC_INCONSISTENT"))
    assert (lrcheck.IN_TENSOR, lrcheck.IN_SBS_NV12) == (enums["SN_LRC_IN_TENSOR"], enums["SN_LRC_IN_SBS_NV12"])
    body = re.search(r"typedef struct sn_lrc_params \{(.*?)\} sn_lrc_params;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.split() for d in body.split(";") if d.strip()]
    ctype = {"float": C.c_float, "int": C.c_int}
    assert [(name, ctype[t]) for t, name in decls] == list(api.SnLrcParams._fields_)
    assert C.sizeof(api.SnLrcParams) == 12
    assert int(re.search(r"#define\s+SN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == api.ABI_VERSION == 4      # 4: SN_ERR_RANGE and the range counts of sn_refine_stats; these structs are as in 3
    lib = api.load_library()
    for sym in ("sn_mirror_pair_i8", "sn_lr_check", "sn_infer_lrc"):
        assert re.search(rf"\bint {sym}\(", HEADER) and hasattr(lib, sym)
    assert lrcheck.OUT_SCALE == pytest.approx(float(re.search(r"float out_scale;\s*/\*\s*([0-9.e-]+)", HEADER).group(1)))


@pytest.mark.parametrize("value", ["-1", "1,-0.5", "nan", "1,2,3", "abc", "inf"])
def test_filelist_rejects_a_bad_lrc_argument_before_any_work(value, capsys):
    from hobot_stereonet_amd import filelist
    with pytest.raises(SystemExit):
        filelist.main(["--model", "none.snw", "--left", "none.list", "--right", "none.list", "--lrc", value])
    assert "--lrc takes TAU_PX[,TAU_REL]" in capsys.readouterr().err
