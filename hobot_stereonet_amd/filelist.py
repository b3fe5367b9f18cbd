"""File-list harness: the Python twin of the reference's offline feeder `StereonetNode::RunImglistFeedInfer`
(stereonet_infer/src/stereonet_node.cpp:820-976) as a plain command line, plus the stereo metrics (EPE, bad-N,
D1) needed to score the output against dataset ground truth.

    python -m hobot_stereonet_amd.filelist --model m.snw --left left.list --right right.list \
        [--gt gt.list] [--out out_dir] [--precision auto|f16|f16x3|fp32] \
        [--ply DIR [--camera fx,fy,cx,cy,baseline_mm]] [--lrc TAU_PX[,TAU_REL]] \
        [--speckle MAX_PX[,DIFF_PX]] [--fill MAX_PX] [--conf MIN] [--smooth RADIUS[,SIGMA[,MIN_VALID]]] \
        [--temporal ALPHA,DELTA_PX[,PERSIST[,LUMA_DELTA]]] [--rectify calib.txt] [--jpeg Q[,ROWS]]
        [--render jpeg[,Q[,ROWS]]|ppm [--render-true-colours] [--render-invalid-black]] \
        [--obstacles PARAMS_FILE] [--ground PARAMS_FILE] [--costmap PARAMS_FILE[,POSES_FILE]] [--elevation PARAMS_FILE[,POSES_FILE]] \
        [--inflate PARAMS_FILE] \
        [--plan PARAMS_FILE] [--rollout PARAMS_FILE]

Per frame i (same order as the reference): read left[i] / right[i] (8-bit colour image) -> BGR -> NV12
(`images.bgr_to_nv12`) -> side-by-side frame -> `sn_infer_sbs_nv12` (split + pre-processing + network on the
GPU) -> int32 wire tensor + float disparity [-> coloured point cloud, `sn_pointcloud_from_raw`, one PLY per pair].  Error behaviour mirrors the reference: an unreadable list, a
missing image or lists of different length stop the run before any inference.  There is no CPU path.

--lrc runs every pair through the left-right consistency check (`sn_infer_lrc`: a second forward on the mirrored pair, then
the check of the two maps): pixels the right eye does not confirm get raw = 0 in every output, <i>.mask.pgm holds the reason per
pixel (lrcheck.REASONS), the metrics are taken over kept pixels with ground truth, and the summary gains "density".

--speckle / --fill run the map (after the check when --lrc is given too) through `sn_filter_raw`: connected components of at most
MAX_PX pixels whose neighbours differ by at most DIFF_PX (default 1) are removed, then row gaps of at most MAX_PX pixels take
the smaller of their two bounding disparities.  The filtered map feeds the metrics, --ply and --out; <i>.filter.pgm holds the
mask (dispfilter.BITS), every record gains "removed" and "filled", the summary their totals and "density".  With ground truth
the metrics cover the measured pixels that survive; the filled ones are interpolation and are scored apart ("filled_epe").

--conf masks every output by the confidence of the soft-argmin distribution (`sn_infer_conf`, no second forward): pixels whose
confidence is below MIN get raw = 0, <i>.conf.pfm holds the confidence, <i>.mask.pgm the reason per pixel (confidence.LOW = 64),
the metrics are taken over kept pixels and the summary gains "density".  With --lrc the public calls are composed with two
forwards, not three: infer_conf unmasked, the mirrored pair through infer, lr_check, conf_mask on its result; the mask is the OR
of the two.  --speckle / --fill run after them, as without it.

--smooth runs the map last of all (after --lrc / --speckle / --fill / --conf) through `sn_smooth_raw`: every pixel takes the
weighted median of its (2 RADIUS + 1)^2 window, weighted by the likeness of the left eye's luma (SIGMA, default 12; 0 = a plain
median), and with MIN_VALID > 0 (default 0) a pixel without a measurement takes it too when that many window pixels hold one.
The guide is the side-by-side NV12 frame the harness holds anyway.  The smoothed map feeds the metrics, --ply and --out;
<i>.smooth.pgm holds the mask (smooth.BITS), every record gains "smoothed" (changed pixels) and "density", the summary their
total and mean.  With ground truth the record gains "smooth_epe": the EPE over the pixels that held a measurement before the
step, before and after it.

--temporal takes the list as ONE clip in list order and runs every map, after --smooth and everything before it, through a
temporal filter (`sn_temporal_push`, one stream): a measurement within DELTA_PX of the pixel's filtered past is blended with it
(weight ALPHA / 256 for the new one), a pixel without one keeps its last value while PERSIST of its last eight inputs held one
(default 2, 0 = never), and with LUMA_DELTA > 0 (default 0) a luma change above it in the left eye stops both.  The filtered
map feeds the metrics, --ply and --out; <i>.temporal.pgm holds the mask (temporal.BITS: a plane of its own), every record
gains "blended", "held" and "density", the summary their totals and mean and "flicker_before" / "flicker_after" (mean frame to
frame change in px over pixels measured in both frames).  With ground truth the record gains "temporal_epe", before and after.

--rectify takes a calibration file (rectify.load_calib: size, left.K / .D / .R, right.K / .D / .R, P, baseline_mm).  The listed
images are then RAW, of the calibration's source size: they are converted to NV12 as always, rectified on the GPU
(`sn_rectify_nv12`) into the side-by-side frame of the model's size, and that frame feeds everything above unchanged.
<i>.rect.ppm holds the rectified frame (both eyes, RGB), --ply takes its camera from the rectifier unless --camera is given,
and the summary gains "valid_left" / "valid_right", the pixels of each eye that have a source.

--jpeg Q[,ROWS] encodes the left eye of every frame (the rectified one with --rectify) on the GPU (`sn_jpeg_encode_nv12`,
quality Q, restart intervals of ROWS MCU rows, default 1; 0 = a single scan) and writes <i>.left.jpg into --out: the node's
left-eye picture, byte for byte the host encoder's stream.  Every record gains "jpeg_bytes".

--render jpeg[,Q[,ROWS]] | ppm writes the reference render node's picture of every frame into --out, made on the GPU from the
FINAL map of the chain and the frame's left eye: the left eye on top, the colour-mapped depth below.  jpeg: <i>.render.jpg by
`sn_render_jpeg` (quality Q, default 95; restart intervals of ROWS MCU rows, default 1); ppm: <i>.render.ppm, the RGB8 canvas of
`sn_render`.  The default is the reference's published picture (its colour map with red and blue swapped, raw == 0 painted like
the farthest depth); --render-true-colours keeps the colour map's own colours, --render-invalid-black paints pixels without a
measurement (raw == 0, what the masks above leave) black.  Every record gains "render_bytes".

--obstacles PARAMS_FILE (obstacles.save_params' `key value` lines) reduces the FINAL map of the chain on the GPU
(`sn_obstacles_from_raw`) to where a robot cannot drive, with --camera or the rectifier's camera as --ply: <i>.grid.pgm, the
occupancy grid seen from above with forward up (0 occupied, 128 unknown, 255 free), and <i>.scan.txt, one `angle range` line per
beam of the laser scan, are written into --out; the summary gains per pair "occupied" and "free" (cells) and "nearest_m" (the
smallest range, null without a return).

--ground PARAMS_FILE (ground.save_params' `key value` lines) fits the ground plane of the FINAL map on the GPU
(`sn_ground_from_raw`), camera as above: <i>.ground.txt (the record: flags, counts, the plane, the mount, pitch and roll) and
<i>.ground.pgm (the labels: no measurement 0, no plane 48, above 96, below 160, ground 255) are written into --out; the summary gains
per pair "ground_found", "height_m", "pitch_deg", "roll_deg" and "inliers".  With --obstacles the grid and the scan use the mount
the fit hands back (the file's own prior where no plane was found) instead of the obstacle file's base_from_cam.

--costmap PARAMS_FILE[,POSES_FILE] (costmap.save_params' `key value` lines; needs --obstacles) treats the list as ONE clip and
accumulates every frame's grid and scan on the GPU (`sn_costmap_push`) into a rolling log-odds map with ray clearing that
travels with the robot.  POSES_FILE holds one `x y yaw` line per pair (metres and radians in the map's fixed frame); without
it every pair stands at the origin.  <i>.costmap.pgm (0 occupied .. 255 free, 128 unknown, world x up) is written into --out;
the summary gains "costmap": per pair "known", "occupied" (cells with positive log-odds), "hit" and "cleared" (cells this frame).

--elevation PARAMS_FILE[,POSES_FILE] (elevation.save_params' `key value` lines) treats the list as ONE clip and fuses every frame's
final map on the GPU (`sn_elevation_push`) into a rolling elevation map with a step-height traversability verdict, at the frame's
pose and, with --ground, under the frame's fitted mount.  <i>.trav.pgm (0 lethal, 255 drivable, 128 unknown, world x up) and
<i>.hi.pgm (the cells' upper heights, 0 unknown) are written into --out; the summary gains "elevation": per pair "known", "lethal"
and "fused" (cells this frame).

--inflate PARAMS_FILE (inflate.save_params' `key value` lines; needs --obstacles with a grid) charges every cell for its distance
to the nearest obstacle on the GPU (`sn_inflate_grid`): of the costmap's grid with --costmap, else of the obstacle grid, with
cell_m taken from the obstacle file.  <i>.inflated.pgm (the cost bytes: 254 lethal, 253 inscribed, 1..252 the fall-off, 0 free,
255 unknown; row y of the grid is row y of the picture) is written into --out; the summary gains "inflate": per pair "lethal",
"inscribed", "inflated", "free" and "unknown".

--plan PARAMS_FILE (navfn.save_params' `key value` lines, with `goal x y` and `start x y` in cells of the inflated grid; needs
--inflate) computes on the GPU (`sn_navfn`) the cost-to-go of every cell of the inflated grid to the goal and the path that follows
it down from the start.  <i>.plan.pgm (the potential scaled to 0..254 by the frame's largest finite value, blocked and unreachable
cells at 255) and <i>.path.txt (one `x y` line per cell, start first) are written into --out; the summary gains "plan": per pair
"flags" (1 goal blocked, 2 start unreachable, 4 path truncated, 8 unconverged: a file
with max_rounds > 0 whose rounds did not finish the field), "reached", "path_cells", "p_start" and "blocked".

--rollout PARAMS_FILE (rollout.save_params' `key value` lines with one `point x y` line per footprint point and an optional
`pose x y yaw` in metres from the corner of the inflated grid; needs --plan) rolls a lattice of velocity commands forward over
the inflated grid on the GPU (`sn_rollout`) and picks the one that ends nearest the goal without its footprint touching an
obstacle.  The pose is the file's, else the centre of the plan's start cell (of cell (0, 0) without a start) at yaw 0; the file's
cell_m must be the grid's.  <i>.rollout.txt (`cmd v w`, `best` and its eight words, then one `X Y heading` line per step in
1/256 cell and 1/65536 turn) is written into --out; the summary gains "rollout": per pair "v", "w" (0 without a valid sample),
"score" (null without one), "valid", "collided", "no_route" and "out_of_window".
"""
import argparse
import json
import os
import sys
from typing import Dict, List, Optional

import numpy as np

from . import images


class FileListError(RuntimeError):
    pass


def read_list(path: str) -> List[str]:
    """One image path per line; every entry must exist (stereonet_node.cpp:832-878)."""
    if not os.path.isfile(path):
        raise FileListError(f"Open file failed: {path}")
    out = []
    with open(path) as f:
        for line in f.read().splitlines():
            name = line.rstrip("\r ")
            if not os.path.exists(name):
                raise FileListError(f"File is not exist! img_name: {name}")
            out.append(name)
    return out


def read_pair_lists(left_list: str, right_list: str):
    left, right = read_list(left_list), read_list(right_list)
    if len(left) != len(right):
        raise FileListError(f"Imgs size error! left_imgs.size: {len(left)}, right_imgs.size: {len(right)}")
    return left, right


# ---- metrics ----------------------------------------------------------------------------------------------
def epe(pred: np.ndarray, gt: np.ndarray, valid: Optional[np.ndarray] = None) -> float:
    """Mean absolute disparity error over the valid pixels (end-point error of a 1-D flow)."""
    err = np.abs(pred.astype(np.float64) - gt.astype(np.float64))
    if valid is not None:
        err = err[valid]
    return float(err.mean()) if err.size else float("nan")


def bad_px(pred: np.ndarray, gt: np.ndarray, thresh: float, valid: Optional[np.ndarray] = None) -> float:
    """Fraction of valid pixels whose error exceeds `thresh` px (SceneFlow/Middlebury bad-N)."""
    err = np.abs(pred.astype(np.float64) - gt.astype(np.float64))
    if valid is not None:
        err = err[valid]
    return float((err > thresh).mean()) if err.size else float("nan")


def d1(pred: np.ndarray, gt: np.ndarray, valid: Optional[np.ndarray] = None) -> float:
    """KITTI 2015 D1: error > 3 px AND > 5 % of the true disparity."""
    p, g = pred.astype(np.float64), gt.astype(np.float64)
    err = np.abs(p - g)
    bad = (err > 3.0) & (err > 0.05 * np.abs(g))
    if valid is not None:
        bad = bad[valid]
    return float(bad.mean()) if bad.size else float("nan")


def score(pred: np.ndarray, gt: np.ndarray, valid: Optional[np.ndarray], dmax: Optional[float] = None) -> Dict[str, float]:
    if dmax is not None:      # the usual protocol: pixels beyond the search range are not scored
        valid = (gt < dmax) if valid is None else (valid & (gt < dmax))
    return {"epe": epe(pred, gt, valid), "bad1": bad_px(pred, gt, 1.0, valid), "bad3": bad_px(pred, gt, 3.0, valid),
            "d1": d1(pred, gt, valid), "valid_px": int(valid.sum()) if valid is not None else int(gt.size)}


# ---- the feeder ---------------------------------------------------------------------------------------------
def run_imglist(engine, left_list: str, right_list: str, out_dir: Optional[str] = None,
                gt_list: Optional[str] = None, log=None, ply_dir: Optional[str] = None, camera=None,
                lrc=None, flt=None, conf: Optional[float] = None, smooth=None, temporal=None, rectify=None,
                jpeg=None, view=None, obstacle=None, ground=None, costmap=None, inflation=None, plan=None, roll=None,
                elevation=None) -> List[dict]:
    """Feeds every (left[i], right[i]) pair through `engine` (api.StereoNetHIP).  Returns one record per frame:
    {"frame_id", "left", "right", "raw" (int32 HxW), "disp" (float32 HxW)[, "metrics"][, "points"]}; with `out_dir` also
    writes <i>.raw.bin, <i>.disp.pfm and <i>.depth.ppm (the render node's colour map); with `ply_dir` <i>.ply, the
    compact point cloud of the pair coloured by its left eye (camera: pointcloud.Camera, default intrinsics if None).
    lrc = (tau_px, tau_rel): the maps are those of engine.infer_lrc (rejected pixels at 0), the record gains "mask" and
    "density", <i>.mask.pgm is written beside the other files and the metrics cover kept pixels only.
    flt = (speckle_max_px, speckle_diff_px, fill_max_px): the maps then pass through engine.filter_raw; the record gains
    "filter_mask", "removed", "filled" and "density" (pixels > 0 after the filter), <i>.filter.pgm is written, "metrics" cover the
    surviving measurements and "metrics_filled" the filled pixels.
    conf = min_conf: the maps are those of engine.infer_conf (pixels below the threshold at 0); the record gains "conf", "mask"
    and "density", <i>.conf.pfm and <i>.mask.pgm are written.  With lrc as well: infer_conf unmasked, infer on the mirrored pair,
    lr_check, conf_mask — two forwards — and "mask" is the OR of the two masks.
    smooth = (radius, sigma_luma, min_valid): the maps then pass through engine.smooth_raw, guided by the frame's left eye; the
    record gains "smooth_mask", "smoothed" (changed pixels) and "density" (pixels > 0 after the step), <i>.smooth.pgm is written,
    and with ground truth "smooth_epe" = {"before", "after", "valid_px"} over the pixels that held a measurement before it.
    temporal = (alpha, delta_px, persist, luma_delta): the list is one clip; the maps pass last through one api.TemporalFilter
    that lives for the call; the record gains "temporal_in" (the map before the step), "temporal_mask", "blended", "held" and
    "density", <i>.temporal.pgm is written, and with ground truth "temporal_epe" as "smooth_epe".
    rectify = a rectify.Calib: the images are raw eyes of its source size; one api.Rectifier lives for the call and turns every
    pair into the rectified side-by-side frame that feeds all of the above; the record gains "rect" (that frame), <i>.rect.ppm is
    written, the record gains "valid_left" / "valid_right", and `camera` defaults to the rectifier's.
    jpeg = (quality, rows_per_slice): the record gains "jpeg" (the left eye's stream from engine.jpeg_encode_nv12) and
    "jpeg_bytes", and <i>.left.jpg is written.
    view = ("jpeg", quality, rows_per_slice, render.RenderParams) or ("ppm", render.RenderParams): the record gains "render" (the
    stream of engine.render_jpeg, or the RGB8 canvas of engine.render, of the final map under the left eye) and "render_bytes",
    and <i>.render.jpg / <i>.render.ppm is written.
    obstacle = an obstacles.ObstacleParams: the record gains "occ", "ranges" and "obstacle_stats" (engine.obstacles of the final
    map, `camera` as for the cloud), "occupied", "free" and "nearest_m"; <i>.grid.pgm and <i>.scan.txt are written.
    ground = a ground.GroundParams: the record gains "ground" (the record of engine.ground of the final map) and "ground_labels",
    "ground_found", "height_m", "pitch_deg", "roll_deg" and "inliers"; <i>.ground.txt and <i>.ground.pgm are written, and the
    obstacle stage takes the record's mount.
    costmap = (costmap.CostmapParams, poses (n, 3) or None), with `obstacle`: the list is one clip; one api.Costmap lives for the
    call and takes every frame's "occ" and "ranges" at the frame's pose (None: the origin); the record gains "costmap" (the int8
    grid), "costmap_q" and "costmap_stats" = {"known", "occupied", "hit", "cleared"}, and <i>.costmap.pgm is written.
    inflation = an inflate.InflateParams whose cell_m is the obstacle grid's, with `obstacle` (gw > 0): engine.inflate of the
    costmap's grid (with `costmap`) or else of "occ"; the record gains "inflated" (the uint8 cost) and "inflate_stats" =
    {"lethal", "inscribed", "inflated", "free", "unknown"}, and <i>.inflated.pgm is written.
    plan = a navfn.NavParams with its goal (and start) in cells, with `inflation`: engine.navfn of "inflated"; the record gains
    "potential" (uint32), "path" (int32 (cells, 2), empty without a start or a route) and "plan_stats" = navfn.STATS' keys, and
    <i>.plan.pgm and <i>.path.txt are written.
    roll = a rollout.RolloutParams with its footprint (and pose), with `plan`: engine.rollout of "inflated" and "potential"; the
    record gains "rollout_best" (uint32 (8,)), "rollout_traj" (int32 (T+1, 3)) and "cmd" = (v, w), (0, 0) without a valid sample,
    and <i>.rollout.txt is written."""
    left, right = read_pair_lists(left_list, right_list)
    gts = read_list(gt_list) if gt_list else None
    if gts is not None and len(gts) != len(left):
        raise FileListError(f"Imgs size error! left_imgs.size: {len(left)}, gt.size: {len(gts)}")
    for d in (out_dir, ply_dir):
        if d:
            os.makedirs(d, exist_ok=True)
    w, h = engine.width, engine.height
    results = []
    tf = engine.temporal_filter(1, *temporal) if temporal is not None else None
    rect = cm = ev = None
    if elevation is not None and elevation[1] is not None and len(elevation[1]) != len(left):
        raise FileListError(f"Poses size error! left_imgs.size: {len(left)}, poses.size: {len(elevation[1])}")
    if costmap is not None:
        if obstacle is None:
            raise FileListError("the costmap needs the obstacle stage")
        if costmap[1] is not None and len(costmap[1]) != len(left):
            raise FileListError(f"Poses size error! left_imgs.size: {len(left)}, poses.size: {len(costmap[1])}")
    if inflation is not None and (obstacle is None or not obstacle.gw):
        raise FileListError("the inflation needs the obstacle stage's grid")
    if plan is not None and inflation is None:
        raise FileListError("the plan needs the inflated grid")
    if roll is not None and plan is None:
        raise FileListError("the rollout needs the plan")
    try:
        if costmap is not None:
            cm = (engine.costmap(obstacle, costmap[0]), costmap[1])
        if elevation is not None:
            ev = (engine.elevation(elevation[0]), elevation[1])
        if rectify is not None:
            rect = engine.rectifier(rectify)
            camera = camera or rect.camera
        _feed(engine, left, right, gts, out_dir, ply_dir, camera, lrc, flt, conf, smooth, tf, log, results, rect, jpeg, view, obstacle, ground, cm,
              inflation, plan, roll, ev)
    finally:
        if cm is not None:
            cm[0].close()
        if ev is not None:
            ev[0].close()
        if rect is not None:
            rect.close()
        if tf is not None:
            tf.close()
    return results


def _feed(engine, left, right, gts, out_dir, ply_dir, camera, lrc, flt, conf, smooth, tf, log, results, rect=None, jpeg=None, view=None,
          obstacle=None, ground=None, cm=None, inflation=None, plan=None, rollp=None, ev=None):
    w, h = engine.width, engine.height
    iw, ih = (rect.src_w, rect.src_h) if rect is not None else (w, h)      # the size of the listed images
    valid = rect.info if rect is not None else None
    for i, (lp, rp) in enumerate(zip(left, right)):
        if log:
            log(f"Feed {i}/{len(left)}")
        eyes = []
        for p in (lp, rp):
            bgr = images.imread_bgr(p)
            if bgr.shape[:2] != (ih, iw):
                raise FileListError(f"BGRToNv12 Fail: {p} is {bgr.shape[1]}x{bgr.shape[0]}, "
                                    f"{'the calibration is for' if rect is not None else 'model input is'} {iw}x{ih}")
            eyes.append(images.bgr_to_nv12(bgr))
        sbs = images.sbs_from_eyes(eyes[0], eyes[1], w, h) if rect is None else rect.rectify(eyes[0], eyes[1])[0]
        cf = None
        if conf is not None and lrc is not None:
            disp, raw, cf = engine.infer_conf(sbs)
            _, raw_m = engine.infer(engine.mirror_pair(engine.preprocess_sbs_nv12(sbs).reshape(6, h, w)))
            raw, mask, _ = engine.lr_check(raw, raw_m.reshape(h, w), lrc[0], lrc[1], True, disp)
            raw, cmask, kept = engine.conf_mask(raw, cf, conf, disp)
            mask = mask | cmask
        elif conf is not None:
            disp, raw, cf, mask, kept = engine.infer_conf(sbs, conf)
        elif lrc is None:
            disp, raw = engine.infer_sbs_nv12(sbs)
        else:
            disp, raw, mask, kept = engine.infer_lrc(sbs, lrc[0], lrc[1])
        masked = lrc is not None or conf is not None
        rec = {"frame_id": str(i), "left": lp, "right": rp, "raw": raw, "disp": disp}
        if rect is not None:
            rec.update(rect=sbs, valid_left=valid["valid_left"], valid_right=valid["valid_right"])
        if jpeg is not None:      # the left half of the side-by-side frame, read in place at pitch 2w
            rec["jpeg"] = engine.jpeg_encode_nv12(sbs, w, h, 2 * w, quality=jpeg[0], rows_per_slice=jpeg[1])[0]
            rec["jpeg_bytes"] = len(rec["jpeg"])
        if masked:
            rec["mask"] = mask
            rec["density"] = float(kept[0]) / float(w * h)
        if cf is not None:
            rec["conf"] = cf
        if flt is not None:
            raw, fmask, counts = engine.filter_raw(raw, flt[0], flt[1], flt[2], disp=disp)
            rec.update(raw=raw, filter_mask=fmask, removed=int(counts[0][1]), filled=int(counts[0][2]),
                       density=float(counts[0][0]) / float(w * h))
        if smooth is not None:
            raw_in, disp_in = raw, disp.copy()
            raw, smask, counts = engine.smooth_raw(raw, sbs, 0, 2 * w, smooth[0], smooth[1], smooth[2], disp=disp)
            rec.update(raw=raw, smooth_mask=smask, smoothed=int(counts[0][1]) + int(counts[0][2]),
                       density=float(counts[0][0]) / float(w * h))
        if tf is not None:
            traw_in, tdisp_in = raw, disp.copy()
            raw, tmask, counts = tf.push(raw, sbs, 0, 2 * w, disp=disp)
            rec.update(raw=raw, temporal_in=traw_in, temporal_mask=tmask, blended=int(counts[0][1]), held=int(counts[0][2]),
                       density=float(counts[0][0]) / float(w * h))
        if view is not None:      # the final map; the left half of the side-by-side frame, read in place at pitch 2w
            if view[0] == "jpeg":
                rec["render"] = engine.render_jpeg(raw, sbs, 2 * w, view[3], quality=view[1], rows_per_slice=view[2])[0]
                rec["render_bytes"] = len(rec["render"])
            else:
                rec["render"] = engine.render(raw, sbs, 2 * w, view[1])
                rec["render_bytes"] = int(rec["render"].size)
        mounts = None
        if ground is not None:        # the final map
            import math
            from . import ground as gnd
            grec, glab = engine.ground(raw, camera, ground)
            pitch, roll = gnd.angles(grec["base_from_cam"])
            rec.update(ground=grec, ground_labels=glab, ground_found=bool(grec["flags"] & gnd.FOUND), height_m=float(grec["plane_cam"][3]),
                       pitch_deg=math.degrees(pitch), roll_deg=math.degrees(roll), inliers=int(grec["inliers"]))
            mounts = grec["base_from_cam"].reshape(1, 12)
        if obstacle is not None:      # the final map
            occ, _, _, ranges, stats = engine.obstacles(raw, camera, obstacle, mounts=mounts)
            near = float(ranges.min()) if ranges.size else float("inf")
            rec.update(occ=occ, ranges=ranges, obstacle_stats=stats, occupied=int(stats[2]), free=int(stats[3]),
                       nearest_m=near if np.isfinite(near) else None)
        if cm is not None:            # the clip's map after this frame
            pose = np.zeros(3) if cm[1] is None else np.asarray(cm[1][i], np.float64)
            grid, _, cstats, q = cm[0].push(pose, occ if obstacle.gw else None, ranges if obstacle.beams else None, want=(True, False, True))
            rec.update(costmap=grid[0], costmap_q=q[0],
                       costmap_stats=dict(zip(("known", "occupied", "hit", "cleared"), (int(v) for v in cstats[0]))))
        if ev is not None:            # the clip's elevation map after this frame, with the frame's fitted mount where there is one
            pose = np.zeros(3) if ev[1] is None else np.asarray(ev[1][i], np.float64)
            trav, hi, _, _, estats, q = ev[0].push(pose, raw, camera or pointcloud.Camera(), mounts=mounts, want=(True, True, False, False, True))
            rec.update(trav=trav[0], elevation_hi=hi[0], elevation_q=q[0],
                       elevation_stats=dict(zip(("known", "lethal", "fused", "points"), (int(v) for v in estats[0]))))
        if inflation is not None:     # of the clip's map, or else of this frame's grid
            from . import inflate as infl
            cost, _, _, istats = engine.inflate(rec["costmap"] if cm is not None else occ, inflation, want=(True, False, False, True))
            rec.update(inflated=cost, inflate_stats=dict(zip(infl.STATS, (int(v) for v in istats))))
        if plan is not None:          # over the costs just made
            from . import navfn as nav
            pot, cells, pstats, _ = engine.navfn(rec["inflated"], plan.goal, plan.start, plan, want=(True, plan.start is not None, True))
            length = min(int(pstats[2]), plan.max_path) if cells is not None else 0
            rec.update(potential=pot, path=cells[:length] if cells is not None else np.zeros((0, 2), np.int32),
                       plan_stats=dict(zip(nav.STATS, (int(v) for v in pstats))))
        if rollp is not None:          # over the costs and the field just made
            from . import api, rollout as ro
            cell = float(np.float32(rollp.cell_m))
            sx, sy = plan.start if plan.start is not None else (0, 0)
            pose = rollp.pose if rollp.pose is not None else ((sx + 0.5) * cell, (sy + 0.5) * cell, 0.0)
            _, best, traj = engine.rollout(rec["inflated"], rec["potential"], api.rollout_pose_q(cell, 0.0, 0.0, pose), rollp,
                                           want=(False, True, True))
            found = not int(best[0]) & ro.NO_VALID
            rec.update(rollout_best=best, rollout_traj=traj, cmd=api.rollout_velocity(rollp, int(best[1])) if found else (0.0, 0.0))
        if ply_dir:
            from . import pointcloud
            pts, cnt = engine.pointcloud(raw, camera, pointcloud.COMPACT, sbs, 2 * w)
            rec["points"] = pointcloud.write_ply(os.path.join(ply_dir, f"{i}.ply"), pts, int(cnt[0]))
        if gts is not None:
            gt, gt_valid = images.read_disparity(gts[i])
            valid = gt_valid
            if masked:
                valid = (mask == 0) if valid is None else (valid & (mask == 0))
            if flt is not None:      # fmask == 0: a measurement that survived both the check (its raw were 0 otherwise) and the filter
                filled = (fmask & 32) != 0
                rec["metrics_filled"] = score(disp, gt, filled if gt_valid is None else (gt_valid & filled), float(engine.dmax))
                valid = (fmask == 0) if gt_valid is None else (gt_valid & (fmask == 0))
            rec["metrics"] = score(disp, gt, valid, float(engine.dmax))
            if smooth is not None:
                held = (raw_in > 0) & (gt < float(engine.dmax))
                if gt_valid is not None:
                    held &= gt_valid
                rec["smooth_epe"] = {"before": epe(disp_in, gt, held), "after": epe(disp, gt, held), "valid_px": int(held.sum())}
            if tf is not None:
                held = (traw_in > 0) & (gt < float(engine.dmax))
                if gt_valid is not None:
                    held &= gt_valid
                rec["temporal_epe"] = {"before": epe(tdisp_in, gt, held), "after": epe(disp, gt, held), "valid_px": int(held.sum())}
        if out_dir:
            raw.tofile(os.path.join(out_dir, f"{i}.raw.bin"))
            images.write_pfm(os.path.join(out_dir, f"{i}.disp.pfm"), disp)
            from . import render
            _, depth = render.disparity_and_depth(raw.view(np.uint32))
            images.write_ppm(os.path.join(out_dir, f"{i}.depth.ppm"), render.colorize_depth(depth)[..., ::-1])
            if jpeg is not None:
                with open(os.path.join(out_dir, f"{i}.left.jpg"), "wb") as f:
                    f.write(rec["jpeg"])
            if view is not None and view[0] == "jpeg":
                with open(os.path.join(out_dir, f"{i}.render.jpg"), "wb") as f:
                    f.write(rec["render"])
            elif view is not None:
                images.write_ppm(os.path.join(out_dir, f"{i}.render.ppm"), rec["render"])
            if ground is not None:
                from . import ground as gnd
                from . import obstacles as obs
                gnd.write_record(os.path.join(out_dir, f"{i}.ground.txt"), rec["ground"])
                obs.write_pgm(os.path.join(out_dir, f"{i}.ground.pgm"), gnd.labels_image(rec["ground_labels"]))
            if obstacle is not None:
                from . import obstacles as obs
                if obstacle.gw:
                    obs.write_pgm(os.path.join(out_dir, f"{i}.grid.pgm"), obs.grid_image(rec["occ"]))
                if obstacle.beams:
                    obs.write_scan(os.path.join(out_dir, f"{i}.scan.txt"), obstacle, rec["ranges"])
            if cm is not None:
                from . import costmap as cmap
                cmap.write_pgm(os.path.join(out_dir, f"{i}.costmap.pgm"), rec["costmap"])
            if ev is not None:
                from . import elevation as elev
                from . import obstacles as obs
                obs.write_pgm(os.path.join(out_dir, f"{i}.trav.pgm"), elev.trav_image(rec["trav"]))
                obs.write_pgm(os.path.join(out_dir, f"{i}.hi.pgm"), elev.height_image(rec["elevation_hi"]))
            if inflation is not None:
                from . import inflate as infl
                infl.write_pgm(os.path.join(out_dir, f"{i}.inflated.pgm"), rec["inflated"])
            if plan is not None:
                from . import navfn as nav
                nav.write_pgm(os.path.join(out_dir, f"{i}.plan.pgm"), rec["potential"])
                nav.write_path(os.path.join(out_dir, f"{i}.path.txt"), rec["path"])
            if rollp is not None:
                from . import rollout as ro
                ro.write_rollout(os.path.join(out_dir, f"{i}.rollout.txt"), rec["cmd"][0], rec["cmd"][1], rec["rollout_best"], rec["rollout_traj"])
            if rect is not None:
                from . import rectify as rct
                images.write_ppm(os.path.join(out_dir, f"{i}.rect.ppm"), rct.sbs_to_rgb(sbs))
            if masked:
                images.write_ppm(os.path.join(out_dir, f"{i}.mask.pgm"), mask)      # 2-D: written as a P5 greymap
            if cf is not None:
                images.write_pfm(os.path.join(out_dir, f"{i}.conf.pfm"), cf)
            if flt is not None:
                images.write_ppm(os.path.join(out_dir, f"{i}.filter.pgm"), fmask)
            if smooth is not None:
                images.write_ppm(os.path.join(out_dir, f"{i}.smooth.pgm"), smask)
            if tf is not None:
                images.write_ppm(os.path.join(out_dir, f"{i}.temporal.pgm"), tmask)
        results.append(rec)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", required=True, help=".snw weight file (the role of hobot_stereonet.hbm)")
    ap.add_argument("--left", required=True)
    ap.add_argument("--right", required=True)
    ap.add_argument("--gt", default=None, help="optional list of ground-truth disparities (.pfm or 16-bit .png)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--precision", choices=["auto", "f16", "f16x3", "fp32"], default="auto")
    ap.add_argument("--device", type=int, default=-1)
    ap.add_argument("--ply", default=None, metavar="DIR", help="write <i>.ply, the pair's coloured point cloud (GPU)")
    ap.add_argument("--camera", default=None, metavar="fx,fy,cx,cy,baseline_mm",
                    help="intrinsics of the rectified left eye for --ply (default: the reference's, centred)")
    ap.add_argument("--lrc", default=None, metavar="TAU_PX[,TAU_REL]",
                    help="left-right consistency check: drop pixels whose right-eye disparity differs by more than "
                         "TAU_PX + TAU_REL * disparity px (one more forward per pair)")
    ap.add_argument("--speckle", default=None, metavar="MAX_PX[,DIFF_PX]",
                    help="remove connected components of at most MAX_PX pixels; neighbours belong together when their "
                         "disparities differ by at most DIFF_PX px (default 1)")
    ap.add_argument("--fill", default=None, metavar="MAX_PX",
                    help="fill row gaps of at most MAX_PX pixels with the smaller bounding disparity (after --speckle)")
    ap.add_argument("--conf", default=None, metavar="MIN",
                    help="drop pixels whose soft-argmin confidence (0..1) is below MIN (no second forward)")
    ap.add_argument("--smooth", default=None, metavar="RADIUS[,SIGMA[,MIN_VALID]]",
                    help="guided weighted median over a (2 RADIUS + 1)^2 window, RADIUS 1..3; SIGMA 0..255 is the luma scale of "
                         "the weights (default 12, 0 = plain median); MIN_VALID > 0 also fills pixels without a measurement "
                         "whose window holds that many (default 0); runs after every other step")
    ap.add_argument("--temporal", default=None, metavar="ALPHA,DELTA_PX[,PERSIST[,LUMA_DELTA]]",
                    help="temporal filter over the list as one clip, after every other step: ALPHA 1..256 is the weight of the "
                         "new measurement in 1/256, DELTA_PX the largest change that is still blended, PERSIST 0..8 (default 2) "
                         "how many of the last eight inputs must be valid to hold a value, LUMA_DELTA 0..255 (default 0 = off) "
                         "the luma change that counts as motion")
    ap.add_argument("--jpeg", default=None, metavar="Q[,ROWS]",
                    help="write <i>.left.jpg, the left eye encoded on the GPU at quality Q with restart intervals of ROWS MCU rows "
                         "(default 1; 0 = a single scan); needs --out")
    ap.add_argument("--render", default=None, metavar="jpeg[,Q[,ROWS]]|ppm",
                    help="write <i>.render.jpg (quality Q, default 95; restart intervals of ROWS MCU rows, default 1) or "
                         "<i>.render.ppm: the left eye over the colour-mapped depth of the final map, made on the GPU; needs --out")
    ap.add_argument("--obstacles", default=None, metavar="PARAMS_FILE",
                    help="write <i>.grid.pgm and <i>.scan.txt: the obstacle grid and the laser scan of the final map, made on the GPU "
                         "with --camera or the rectifier's camera; needs --out")
    ap.add_argument("--ground", default=None, metavar="PARAMS_FILE",
                    help="write <i>.ground.txt and <i>.ground.pgm: the ground plane of the final map, the mount it implies and the "
                         "per-pixel labels, made on the GPU with --camera or the rectifier's camera; --obstacles then uses that mount; "
                         "needs --out")
    ap.add_argument("--costmap", default=None, metavar="PARAMS_FILE[,POSES_FILE]",
                    help="write <i>.costmap.pgm: the list is one clip whose grids and scans accumulate on the GPU into a rolling "
                         "log-odds map with ray clearing; POSES_FILE: one `x y yaw` line per pair (default: the origin); needs --obstacles")
    ap.add_argument("--elevation", default=None, metavar="PARAMS_FILE[,POSES_FILE]",
                    help="write <i>.trav.pgm and <i>.hi.pgm: the list is one clip whose maps are fused on the GPU into a rolling "
                         "elevation map with a step-height traversability verdict; POSES_FILE: one `x y yaw` line per pair (default: "
                         "the origin); with --ground the frame's fitted mount is used; needs --out")
    ap.add_argument("--inflate", default=None, metavar="PARAMS_FILE",
                    help="write <i>.inflated.pgm: the cost of every cell after inflation by the robot's radius on the GPU, of the "
                         "costmap's grid with --costmap, else of the obstacle grid; needs --obstacles with a grid")
    ap.add_argument("--plan", default=None, metavar="PARAMS_FILE",
                    help="write <i>.plan.pgm and <i>.path.txt: the cost-to-go of every cell of the inflated grid to the file's goal "
                         "and the path from its start, in cells, on the GPU; needs --inflate")
    ap.add_argument("--rollout", default=None, metavar="PARAMS_FILE",
                    help="write <i>.rollout.txt: the velocity command whose arc ends nearest the plan's goal without the file's "
                         "footprint touching an obstacle of the inflated grid, and that arc, on the GPU; needs --plan")
    ap.add_argument("--render-true-colours", action="store_true", help="--render: the colour map's own colours, not the reference's R/B swap")
    ap.add_argument("--render-invalid-black", action="store_true", help="--render: pixels without a measurement (raw == 0) are black")
    ap.add_argument("--rectify", default=None, metavar="CALIB",
                    help="calibration file (size, left.K/.D/.R, right.K/.D/.R, P, baseline_mm): the listed images are raw, of "
                         "its source size, and are rectified on the GPU to the model's size before everything else")
    args = ap.parse_args(argv)
    from . import api, pointcloud
    cam = None
    if args.camera:
        v = [float(t) for t in args.camera.split(",")]
        if len(v) != 5:
            ap.error("--camera takes fx,fy,cx,cy,baseline_mm")
        cam = pointcloud.Camera(fx=v[0], fy=v[1], cx=v[2], cy=v[3], baseline_mm=v[4])
    lrc = None
    if args.lrc:
        try:
            v = [float(t) for t in args.lrc.split(",")]
        except ValueError:
            v = []
        if len(v) not in (1, 2) or not all(np.isfinite(t) and t >= 0 for t in v):
            ap.error("--lrc takes TAU_PX[,TAU_REL], both finite and >= 0")
        lrc = (v[0], v[1] if len(v) == 2 else 0.0)
    conf = None
    if args.conf is not None:
        try:
            conf = float(args.conf)
        except ValueError:
            conf = -1.0
        if not (np.isfinite(conf) and 0.0 <= conf <= 1.0):
            ap.error("--conf takes MIN, a confidence in 0..1")
    flt = None
    if args.speckle is not None or args.fill is not None:
        smax, sdiff, fmax = 0, 1.0, 0
        if args.speckle is not None:
            t = args.speckle.split(",")
            try:
                smax, sdiff = int(t[0]), float(t[1]) if len(t) == 2 else 1.0
            except ValueError:
                smax = -1
            if len(t) not in (1, 2) or smax < 1 or smax > 2 ** 31 - 1 or not (np.isfinite(sdiff) and sdiff >= 0):
                ap.error("--speckle takes MAX_PX[,DIFF_PX]: an integer >= 1 and a finite difference >= 0")
        if args.fill is not None:
            try:
                fmax = int(args.fill)
            except ValueError:
                fmax = -1
            if fmax < 1 or fmax > 2 ** 31 - 1:
                ap.error("--fill takes MAX_PX, an integer >= 1")
        flt = (smax, sdiff, fmax)
    smooth = None
    if args.smooth is not None:
        try:
            v = [int(t) for t in args.smooth.split(",")]
        except ValueError:
            v = []
        v += [12, 0][len(v) - 1:] if 1 <= len(v) <= 3 else []
        if len(v) != 3 or not (1 <= v[0] <= 3 and 0 <= v[1] <= 255 and 0 <= v[2] <= (2 * v[0] + 1) ** 2):
            ap.error("--smooth takes RADIUS[,SIGMA[,MIN_VALID]]: integers, 1..3, 0..255 and 0..(2 RADIUS + 1)^2")
        smooth = tuple(v)
    temporal = None
    if args.temporal is not None:
        t = args.temporal.split(",")
        try:
            v = [int(t[0]), float(t[1])] + [int(x) for x in t[2:]]
        except (ValueError, IndexError):
            v = []
        v += [2, 0][len(v) - 2:] if 2 <= len(v) <= 4 else []
        if len(v) != 4 or not (1 <= v[0] <= 256 and np.isfinite(v[1]) and v[1] >= 0 and 0 <= v[2] <= 8 and 0 <= v[3] <= 255):
            ap.error("--temporal takes ALPHA,DELTA_PX[,PERSIST[,LUMA_DELTA]]: 1..256, a finite difference >= 0, 0..8 and 0..255")
        temporal = tuple(v)
    calib = None
    if args.rectify is not None:
        from . import rectify as rct
        try:
            calib = rct.load_calib(args.rectify)
        except (OSError, ValueError) as e:
            ap.error(f"--rectify takes a calibration file: {e}")
        if not calib.ok():
            ap.error("--rectify takes a calibration file: sizes even and 2..8192, every value finite, focal lengths and baseline > 0")
    jpg = None
    if args.jpeg is not None:
        try:
            parts = [int(v) for v in args.jpeg.split(",")]
            jpg = (parts[0], parts[1] if len(parts) > 1 else 1)
            if len(parts) > 2 or not args.out:
                raise ValueError
        except ValueError:
            ap.error("--jpeg takes Q[,ROWS] (integers) and needs --out")
    rnd = None
    if args.render is not None:
        from . import render as rnd_mod
        prm = rnd_mod.RenderParams(true_colours=int(args.render_true_colours), invalid_black=int(args.render_invalid_black))
        t = args.render.split(",")
        try:
            v = [int(x) for x in t[1:]]
            if t[0] == "jpeg" and len(v) <= 2 and args.out:
                rnd = ("jpeg", v[0] if v else 95, v[1] if len(v) > 1 else 1, prm)
            elif t[0] == "ppm" and not v and args.out:
                rnd = ("ppm", prm)
            else:
                raise ValueError
        except ValueError:
            ap.error("--render takes jpeg[,Q[,ROWS]] (integers) or ppm, and needs --out")
    elif args.render_true_colours or args.render_invalid_black:
        ap.error("--render-true-colours and --render-invalid-black need --render")
    obstacle = None
    if args.obstacles is not None:
        from . import obstacles as obs
        try:
            obstacle = obs.load_params(args.obstacles)
            why = obs.check(obstacle) or (None if args.out else "needs --out")
            if obstacle.beams:
                obs.beam_edges(obstacle)
            if why:
                raise ValueError(why)
        except (OSError, ValueError) as e:
            ap.error(f"--obstacles {args.obstacles}: {e}")
    gparams = None
    if args.ground is not None:
        from . import ground as gnd
        try:
            gparams = gnd.load_params(args.ground)
            why = gnd.check(gparams) or (None if args.out else "needs --out")
            if why:
                raise ValueError(why)
        except (OSError, ValueError) as e:
            ap.error(f"--ground {args.ground}: {e}")
    cmap = None
    if args.costmap is not None:
        from . import costmap as cmod
        if obstacle is None:
            ap.error("--costmap needs --obstacles")
        try:
            files = args.costmap.split(",")
            if len(files) > 2:
                raise ValueError("takes PARAMS_FILE[,POSES_FILE]")
            cparams = cmod.load_params(files[0])
            why = cmod.check(cparams, obstacle)
            if why:
                raise ValueError(why)
            cposes = cmod.load_poses(files[1]) if len(files) == 2 else None
            for pose in (cposes if cposes is not None else []):
                cmod.pose_q(cparams, obstacle, pose)
            cmap = (cparams, cposes)
        except (OSError, ValueError) as e:
            ap.error(f"--costmap {args.costmap}: {e}")
    elevation = None
    if args.elevation is not None:
        from . import costmap as cmod
        from . import elevation as emod
        try:
            files = args.elevation.split(",")
            if len(files) > 2:
                raise ValueError("takes PARAMS_FILE[,POSES_FILE]")
            eparams = emod.load_params(files[0])
            why = emod.check(eparams) or (None if args.out else "needs --out")
            if why:
                raise ValueError(why)
            eposes = cmod.load_poses(files[1]) if len(files) == 2 else None
            for pose in (eposes if eposes is not None else []):
                emod.pose_q(eparams, pose)
            elevation = (eparams, eposes)
        except (OSError, ValueError) as e:
            ap.error(f"--elevation {args.elevation}: {e}")
    inflation = None
    if args.inflate is not None:
        import dataclasses
        from . import inflate as imod
        if obstacle is None or not obstacle.gw:
            ap.error("--inflate needs --obstacles with a grid")
        try:
            inflation = dataclasses.replace(imod.load_params(args.inflate), cell_m=obstacle.cell_m)
            why = imod.check(inflation)
            if why:
                raise ValueError(why)
            imod.table(inflation)
        except (OSError, ValueError) as e:
            ap.error(f"--inflate {args.inflate}: {e}")
    plan = None
    if args.plan is not None:
        from . import navfn as nmod
        if inflation is None:
            ap.error("--plan needs --inflate")
        try:
            plan = nmod.load_params(args.plan)
            why = nmod.check(plan)
            if why:
                raise ValueError(why)
            if plan.start is not None and plan.max_path == 0:
                raise ValueError("a start needs max_path > 0")
        except (OSError, ValueError) as e:
            ap.error(f"--plan {args.plan}: {e}")
    roll = None
    if args.rollout is not None:
        from . import rollout as rmod
        if plan is None:
            ap.error("--rollout needs --plan")
        try:
            roll = rmod.load_params(args.rollout)
            rmod.tables(roll)                      # every refusal of the stage, before the first pair is read
            if np.float32(roll.cell_m) != np.float32(inflation.cell_m):
                raise ValueError("cell_m is not the inflated grid's")
            if roll.pose is not None:
                rmod.pose_q(roll.cell_m, 0.0, 0.0, roll.pose)
        except (OSError, ValueError) as e:
            ap.error(f"--rollout {args.rollout}: {e}")
    prec = {"auto": api.PREC_AUTO, "f16": api.PREC_F16, "f16x3": api.PREC_F16X3, "fp32": api.PREC_FP32}[args.precision]
    try:
        read_pair_lists(args.left, args.right)          # fail on the lists before touching the GPU
        with api.StereoNetHIP(args.model, device=args.device, precision=prec) as eng:
            recs = run_imglist(eng, args.left, args.right, args.out, args.gt, log=lambda s: print(s, file=sys.stderr),
                               ply_dir=args.ply, camera=cam, lrc=lrc, flt=flt, conf=conf, smooth=smooth, temporal=temporal, rectify=calib,
                               jpeg=jpg, view=rnd, obstacle=obstacle, ground=gparams, costmap=cmap, inflation=inflation, plan=plan, roll=roll,
                               elevation=elevation)
    except (FileListError, ValueError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 5
    summary = {"frames": len(recs)}
    if calib is not None and recs:
        summary["valid_left"], summary["valid_right"] = recs[0]["valid_left"], recs[0]["valid_right"]
    if jpg is not None and recs:
        summary["jpeg_bytes"] = int(sum(r["jpeg_bytes"] for r in recs))
    if rnd is not None and recs:
        summary["render_bytes"] = int(sum(r["render_bytes"] for r in recs))
    if obstacle is not None and recs:
        for k in ("occupied", "free", "nearest_m"):
            summary[k] = [r[k] for r in recs]
    if cmap is not None and recs:
        summary["costmap"] = {k: [r["costmap_stats"][k] for r in recs] for k in ("known", "occupied", "hit", "cleared")}
    if elevation is not None and recs:
        summary["elevation"] = {k: [r["elevation_stats"][k] for r in recs] for k in ("known", "lethal", "fused")}
    if inflation is not None and recs:
        from . import inflate as imod
        summary["inflate"] = {k: [r["inflate_stats"][k] for r in recs] for k in imod.STATS}
    if plan is not None and recs:
        from . import navfn as nmod
        summary["plan"] = {k: [r["plan_stats"][k] for r in recs] for k in nmod.STATS}
    if roll is not None and recs:
        bests = [[int(x) for x in r["rollout_best"]] for r in recs]
        summary["rollout"] = {"v": [r["cmd"][0] for r in recs], "w": [r["cmd"][1] for r in recs],
                              "score": [None if b[0] & 1 else b[2] | b[3] << 32 for b in bests], "valid": [b[4] for b in bests],
                              "collided": [b[5] for b in bests], "no_route": [b[6] for b in bests], "out_of_window": [b[7] for b in bests]}
    if gparams is not None and recs:
        for k in ("ground_found", "height_m", "pitch_deg", "roll_deg", "inliers"):
            summary[k] = [r[k] for r in recs]
    if args.gt and recs:
        for k in ("epe", "bad1", "bad3", "d1"):
            summary[k] = float(np.nanmean([r["metrics"][k] for r in recs]))
    if args.gt and flt is not None and recs:
        summary["filled_epe"] = float(np.nanmean([r["metrics_filled"]["epe"] for r in recs]))
    if flt is not None and recs:
        summary["removed"] = int(sum(r["removed"] for r in recs))
        summary["filled"] = int(sum(r["filled"] for r in recs))
    if smooth is not None and recs:
        summary["smoothed"] = int(sum(r["smoothed"] for r in recs))
        if args.gt:
            summary["smooth_epe_before"] = float(np.nanmean([r["smooth_epe"]["before"] for r in recs]))
            summary["smooth_epe_after"] = float(np.nanmean([r["smooth_epe"]["after"] for r in recs]))
    if temporal is not None and recs:
        from . import temporal as tmp
        scale = float(tmp.wire_scale(eng.out_scale))
        summary["blended"] = int(sum(r["blended"] for r in recs))
        summary["held"] = int(sum(r["held"] for r in recs))
        summary["flicker_before"] = tmp.flicker(np.stack([r["temporal_in"] for r in recs])) * scale
        summary["flicker_after"] = tmp.flicker(np.stack([r["raw"] for r in recs])) * scale
        if args.gt:
            summary["temporal_epe_before"] = float(np.nanmean([r["temporal_epe"]["before"] for r in recs]))
            summary["temporal_epe_after"] = float(np.nanmean([r["temporal_epe"]["after"] for r in recs]))
    if (lrc is not None or flt is not None or conf is not None or smooth is not None or temporal is not None) and recs:
        summary["density"] = float(np.mean([r["density"] for r in recs]))
    print(json.dumps(summary))
    return 0


if __name__ == "__main__":
    sys.exit(main())
