"""The domain the post-processing stages are judged on: the geometries sn_create accepts that stand beside a constant of a
kernel (a wave, a tile, a segment, a vector width, a look-ahead), the inputs of every stage at such a geometry, the settings that
reach every kernel instantiation, the numpy twins' answers, and the calls the header refuses.  tests/test_postproc_domain.py
checks the premises on the CPU (the twins against the plain loops of tests/golden/plain_refs.py, the mask values and counters
the inputs must produce, the refusal table against the contract); tests/test_gpu_postproc_geometry.py runs every stage on the
MI355X and compares bit for bit.  Nothing here touches a GPU."""
import dataclasses
import functools

import numpy as np

from hobot_stereonet_amd import (api, confidence, dispfilter, ground, lrcheck, obstacles, pointcloud, rectify, render, smooth,
                                 spec, temporal)

N = 3                                # maps per call
DMAX = 16                            # the smallest dmax a model file may carry (weights.save_snw: a multiple of 16, >= 16)
IMAX, IMIN = 2 ** 31 - 1, -2 ** 31

# (w, h) -> the constant it stands beside.  csrc names: kFltTW x kFltTH = kSmTW x kSmTH = 64 x 16 (sn_dispfilter.hpp, sn_smooth.hpp),
# 256-column segments (k_lr_check, k_pc_organised, k_gr_score), kPcTile = 4096 samples (sn_pointcloud.hpp), kObAhead = 4 rows
# (sn_obstacles.hpp), kGrRows = 8 sample rows of the lower half (sn_ground.hpp), the W & 3 / W & 15 vector forms (k_temporal,
# k_flt_apply, k_mirror_pair, k_render, k_gr_labels), k_render's 4 x 2-pixel items.
GEOMETRIES = {
    (1, 1): "degenerate: one pixel; no vector form, every halo outside the image, no second render row, one chroma row",
    (2, 2): "degenerate: below a 4-pixel vector; the smallest NV12 canvas; two ground samples",
    (1, 40): "degenerate: W = 1, one lane per row, every horizontal border a seam",
    (70, 1): "degenerate: one row: the smoothing halo lies outside, a render item has no second row, (H+1)/2 = 1 chroma row",
    (5, 3): "degenerate: the network domain's smallest odd shape; W & 3 = 1, H below kObAhead",
    (63, 15): "64 x 16 tile, one below: one partial tile, lane 63 idle (the 2ull << lane masks)",
    (64, 16): "64 x 16 tile, exact: no seam at all (k_flt_seam without borders); W & 15 = 0; 8 ground sample rows = kGrRows",
    (65, 17): "64 x 16 tile, one above: remainders of one column and one row; 9 ground sample rows = kGrRows + 1",
    (255, 3): "256-column segment, one below",
    (256, 2): "256-column segment, exact; two rows (one 4 x 2 render item high)",
    (257, 5): "256-column segment, one above; H = kObAhead + 1",
    (65, 63): "compact tile: 4095 samples = kPcTile - 1",
    (64, 64): "compact tile: 4096 samples = kPcTile; four tile rows without a remainder",
    (241, 17): "compact tile: 4097 samples = kPcTile + 1",
    (129, 33): "several tiles with remainders both ways (2 x 2 full tiles, +1 column, +1 row)",
    (20, 6): "W % 4 == 0 but W % 16 != 0: the 4-pixel form without the 16-byte one",
    (12, 4): "H = kObAhead exactly (a column walk whose look-ahead ends on the last row); W % 4 == 0 below 16",
}
DEGENERATE = ((1, 1), (2, 2), (1, 40), (70, 1), (5, 3))
FULL = tuple(g for g in GEOMETRIES if g[0] >= 63 and g[1] >= 15)      # where every mask value and counter must occur

CAM = pointcloud.Camera(fx=20.0, fy=20.0, baseline_mm=120.0)          # the principal point at the map's centre
OBSTACLE = obstacles.ObstacleParams(x_min_m=0.0, y_min_m=-2.0, cell_m=0.125, gw=16, gh=32, z_floor_m=-1.0, z_lo_m=0.0, z_hi_m=1.0,
                                    min_obstacle_hits=2, min_ground_hits=1, beams=18, angle_min_rad=-0.72, angle_increment_rad=0.08,
                                    range_min_m=0.1, range_max_m=0.6)      # the outer beams' nearest points lie beyond range_max_m
GROUND = ground.GroundParams(hypotheses=48, seed=5, refits=2, tol_px=0.5, min_inliers=8, min_area=2, max_tilt_rad=1.5,
                             height_min_m=0.01, height_max_m=100.0)
SRC = (48, 32)                       # the rectifier's source size

# stage -> its settings.  Every tuple is the stage's own parameter list (see `want`).
SETTINGS = {
    "depth": [(False,), (True,)],                                                              # want_disp
    "pointcloud": [(lay, step, col) for lay in (pointcloud.ORGANISED, pointcloud.COMPACT) for step in (1, 2, 3, 4) for col in (0, 1)],
    "mirror": [()],
    "lr_check": [(1.0, 0.0, False), (0.5, 0.02, True)],                                        # tau_px, tau_rel, mirrored
    "conf_mask": [(0.5,)],
    "filter": [(6, 1.0, 0), (0, 1.0, 16), (40, 0.5, 16)],                                      # PARAMS of tests/test_gpu_dispfilter.py
    "smooth": [(r, s, m) for r in (1, 2, 3) for s in (0, 12) for m in (0, 3)],                 # radius, sigma_luma, min_valid
    "temporal": [(64, 1.0, 1, 24), (64, 1.0, 1, 0)],                                           # alpha, delta_px, persist, luma_delta
    "render": [(fmt, lay) for fmt in (render.RGB8, render.NV12) for lay in (render.STACK, render.DEPTH)],
    "rectifier": [()],
    "obstacles": [("rle",), ("plain",)],                                                       # SN_OBSTACLE_RLE unset / 0
    "ground": [()],
}
# The values each setting's mask (labels, occupancy) must take over FULL, as tests/test_gpu_temporal.py SETTINGS states its own
MASK_VALUES = {
    ("lr_check", (1.0, 0.0, False)): {0, 1, 2, 4, 8}, ("lr_check", (0.5, 0.02, True)): {0, 1, 2, 4, 8},
    ("conf_mask", (0.5,)): {0, 1, 64},
    ("filter", (6, 1.0, 0)): {0, 1, 16}, ("filter", (0, 1.0, 16)): {0, 1, 33}, ("filter", (40, 0.5, 16)): {0, 1, 16, 33, 48},
    **{("smooth", (r, s, 0)): {0, 1, 128} for r in (1, 2, 3) for s in (0, 12)},
    **{("smooth", (r, s, 3)): {0, 1, 128, 129} for r in (1, 2, 3) for s in (0, 12)},
    ("temporal", (64, 1.0, 1, 24)): {0, 1, 2, 5, 8, 9, 16}, ("temporal", (64, 1.0, 1, 0)): {0, 1, 2, 5, 16},
    ("obstacles", ("rle",)): {-1, 0, 100}, ("obstacles", ("plain",)): {-1, 0, 100},
    ("ground", ()): {0, 1, 2, 3},
}
MASK_OF = {"lr_check": "mask", "conf_mask": "mask", "filter": "mask", "smooth": "mask", "temporal": "mask", "obstacles": "occ",
           "ground": "labels"}
COUNTERS_OF = {"lr_check": "kept", "conf_mask": "kept", "filter": "counts", "smooth": "counts", "temporal": "counts",
               "pointcloud": "counts", "obstacles": "stats"}


def refusal(stage, setting, w, h):
    """None, or the words of include/stereonet_hip.h under which the call (for sn_rectify: the create) is SN_ERR_ARG at w x h."""
    if stage == "filter" and setting[0] > h * w:
        return "sn_filter_raw: speckle_max_px outside 0..H*W"
    if stage == "render" and setting[0] == render.NV12 and (w | h) & 1:
        return "sn_render, SN_RENDER_NV12: W and H must be even"
    if stage == "rectifier" and (w % 4 or h % 2):
        return "sn_rectify_create: W % 4 != 0 or an odd H is SN_ERR_ARG"
    if stage == "ground" and w * (h - h // 2) < 3:
        return "sn_ground_from_raw: a region that ... holds fewer than three samples (all four 0: the lower half, h = H - H/2)"
    if stage == "pointcloud" and setting[1] not in (1, 2, 4):
        return "sn_pointcloud_from_raw: step not 1/2/4"
    return None


REFUSALS = {(st, s, g): refusal(st, s, *g) for st, ss in SETTINGS.items() for s in ss for g in GEOMETRIES if refusal(st, s, *g)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def inputs(w, h):
    """Every stage's inputs at w x h, built as the stages' own GPU tests build theirs and never written to: `l` and `r`, int32
    (N, h, w) around ONE smooth surface (a floor that comes nearer down the image, 2 .. 7 px, so that frames of a stream blend,
    the eyes agree and a plane fits), about a quarter of the pixels <= 0 with a few negatives, the corner values in the first
    and last pixels where the map has room; an NV12 guide whose pitch is not the width (noise in the chroma rows and beside the
    luma) and the int8 tensor whose channel 0 carries the same luma; a confidence map with a NaN; random bits for `disp`."""
    rng = np.random.default_rng(1000 * w + h)
    S = float(lrcheck.wire_scale())
    surf = 2.0 + 5.0 * np.arange(h)[:, None] / max(h - 1, 1) + np.cumsum(rng.normal(0, 0.03, (h, w)), -1)
    maps = []
    for _ in range(2):
        m = np.rint(np.clip(surf[None] + rng.normal(0, 0.3, (N, h, w)), 0.01, None) / S).astype(np.int32)
        m[rng.random(m.shape) < 0.22] = 0
        m[rng.random(m.shape) < 0.03] = -7
        maps.append(m)
    l, r = maps
    if w >= 63 and h >= 15:
        l[1, 4:11, 20:38] = 0      # a hole wider than fill_max_px = 16 and than a 7 x 7 window: pixels that stay invalid
    if w >= 3:
        l[1, ::2, -1] = 700        # 0.35 px in the last column: the partner's two taps are the row's last two pixels
    if h * w >= 4:
        l[0].reshape(-1)[:4] = [IMIN, 0, 1, IMAX]
        r[0].reshape(-1)[:3] = [IMAX, IMIN, 1]
    if h * w >= 8:
        l[-1].reshape(-1)[-4:] = [IMAX, 1, 0, IMIN]
        r[-1].reshape(-1)[-2:] = [0, 1]
    conf = rng.random(l.shape, dtype=np.float32)
    conf.reshape(-1)[1] = np.nan
    disp0 = rng.integers(0, 2 ** 32, l.shape, dtype=np.uint32).view(np.float32)
    pitch = w + (w & 1) + 2
    nv = rng.integers(0, 256, (N, h + (h + 1) // 2, pitch), dtype=np.uint8)
    luma = smooth.luma_from_nv12(nv, w, h, pitch, N)
    x = rng.integers(-128, 128, (N, 6, h, w), dtype=np.int8)
    x[:, 0] = (luma ^ np.uint8(0x80)).view(np.int8)
    c = {"l": l, "r": r, "r_mirrored": np.ascontiguousarray(r[..., ::-1]), "conf": conf, "disp0": disp0, "nv": nv, "pitch": pitch,
         "luma": luma, "x": x}
    if refusal("rectifier", (), w, h) is None:
        sw, sh = SRC
        c["calib"] = rectify.synthetic_rig(sw, sh, w, h, sw + w)
        c["src_pitch"] = 2 * sw + 16
        c["src"] = rng.integers(0, 256, (N, sh + sh // 2, c["src_pitch"]), dtype=np.uint8)      # side-by-side frames, noise beside them
    return _freeze(c)


def depth_twin(raw, out_scale):
    """Parse's float / double mix, as tests/test_gpu_parity.py writes it -> (depth, disparity)"""
    f, B = np.float32(527.1931762695312), np.float32(119.89382172)
    dis = raw.astype(np.float32) * np.float32(out_scale)
    with np.errstate(divide="ignore"):
        depth = (np.float64(f * B) / (dis.astype(np.float64) * 16.0 * 12.0) / 1000.0).astype(np.float32)
    return depth, dis * np.float32(16.0) * np.float32(12.0)


def temporal_ids(push):
    """the two pushes of the temporal case: maps 0, 1, 2 to streams 0, 1, 0, then 1, 0, 1: both states are read back"""
    return [0, 1, 0] if push == 0 else [1, 0, 1]


@functools.lru_cache(maxsize=None)
def want(stage, setting, w, h, out_scale=spec.OUT_SCALE):
    """name -> array: what the numpy twin says the call writes (float maps as they are; compare their bits)."""
    assert refusal(stage, setting, w, h) is None, (stage, setting, w, h)
    c = inputs(w, h)
    l, r, disp0 = c["l"], c["r"], c["disp0"]
    S32 = dispfilter.wire_scale(out_scale)
    if stage == "depth":
        depth, disp = depth_twin(l, out_scale)
        out = {"depth": depth, "disp": disp} if setting[0] else {"depth": depth}
    elif stage == "pointcloud":
        layout, step, colour = setting
        pts, counts = pointcloud.reference(l, dataclasses.replace(CAM, step=step), layout, c["nv"] if colour else None,
                                           c["pitch"] if colour else 0, out_scale)
        out = {"points": pts, "counts": counts}
    elif stage == "mirror":
        out = {"out": lrcheck.mirror_pair(c["x"])}
    elif stage == "lr_check":
        tau_px, tau_rel, mirrored = setting
        o, m, k = lrcheck.reference(l, c["r_mirrored"] if mirrored else r, tau_px, tau_rel, mirrored, out_scale)
        out = {"out": o, "mask": m, "kept": k, "disp": np.where(m != 0, np.uint32(0), _bits(disp0)).view(np.float32)}
    elif stage == "conf_mask":
        o, m, k = confidence.mask(l, c["conf"], setting[0])
        out = {"out": o, "mask": m, "kept": k, "disp": np.where(m != 0, np.uint32(0), _bits(disp0)).view(np.float32)}
    elif stage == "filter":
        o, m, k = dispfilter.reference(l, *setting, out_scale=out_scale)
        val = np.where(o > 0, o.astype(np.float32) * S32, np.float32(0))
        out = {"out": o, "mask": m, "counts": k, "disp": np.where(m != 0, _bits(val), _bits(disp0)).view(np.float32)}
    elif stage == "smooth":
        radius, sigma, min_valid = setting
        o, m, k = smooth.reference(l, c["luma"] if sigma else None, radius, sigma, min_valid, out_scale=out_scale)
        out = {"out": o, "mask": m, "counts": k, "disp": smooth.expected_disp(disp0, o, m, out_scale)}
    elif stage == "temporal":
        states, out = {}, {}
        for push, raw in enumerate((l, r)):
            o, m, k = temporal.reference(raw, c["luma"] if setting[3] else None, setting, temporal_ids(push), states, out_scale)
            out.update({f"out{push}": o, f"mask{push}": m, f"counts{push}": k,
                        f"disp{push}": temporal.expected_disp(disp0, raw, o, out_scale)})
    elif stage == "render":
        fmt, layout = setting
        out = {"out": render.canvas(l, c["nv"], c["pitch"], render.RenderParams(layout=layout), fmt)}
    elif stage == "rectifier":
        sbs = rectify.reference(c["calib"], w, h, c["src"], None, c["src_pitch"], N)
        out = {"sbs": sbs, "tensor": rectify.tensor_from_sbs(sbs)}
    elif stage == "obstacles":
        names = ("occ", "hits", "height", "ranges", "stats")
        out = dict(zip(names, obstacles.reference(l, CAM, OBSTACLE, edges=api.beam_edges(OBSTACLE), out_scale=out_scale)))
    elif stage == "ground":
        rec, lab = ground.reference(l, CAM, GROUND, gate_q16=api.ground_gate(CAM, GROUND, w, h), out_scale=out_scale)
        out = {"records": rec, "labels": lab}
    else:
        raise KeyError(stage)
    return _freeze(out)


def comparable(stage, setting, d):
    """The outputs as they are compared: float arrays as their bits, a COMPACT cloud cut to zeros past each map's count (the
    header leaves those rows unspecified), ground records as their bytes."""
    out = {}
    for name, a in d.items():
        a = np.ascontiguousarray(a)
        if stage == "pointcloud" and name == "points" and setting[0] == pointcloud.COMPACT:
            a = a.copy()
            for k, cnt in enumerate(d["counts"]):
                a[k, int(cnt):] = 0
        if a.dtype == np.float32:
            a = a.view(np.uint32)
        elif a.dtype.names:
            a = a.view(np.uint8)
        out[name] = a
    return out


def differing(stage, setting, got, wanted):
    """-> {name: number of differing elements} over the wanted outputs (a missing or mis-shaped one counts whole)"""
    g, t = comparable(stage, setting, got), comparable(stage, setting, wanted)
    bad = {}
    for name, a in t.items():
        b = g.get(name)
        if b is None or b.shape != a.shape or b.dtype != a.dtype:
            bad[name] = a.size
        elif not np.array_equal(a, b):
            bad[name] = int((a != b).sum())
    return bad
