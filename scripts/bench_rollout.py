#!/usr/bin/env python3
"""Times the trajectory rollout (sn_rollout) on the navigation function bench's window: 400 x 400 cells of 0.05 m, the costmap
stage's own grids along the walk of scripts/bench_costmap.py inflated at R = 8, the potential sn_navfn makes of them for a goal
near the far edge, the robot at the centre of its window heading for it.  S = 21 x 41 samples, T = 20 steps over 2 s, the
outline of a 0.6 x 0.4 m rectangle at the finest spacing that stays within SN_ROLLOUT_MAX_POINTS (half a cell needs 80 points,
so the bench takes one cell: 40 points).  Device buffers on a caller stream, device events, 50 calls after 5 warm-up, at batch
64 and at batch 1, with all outputs, with best alone and with samples alone; and all outputs again at the 64 points the contract
allows (a spacing of 0.032 m).

In the same run, on the same box: sn_navfn (fixed rounds, the potential alone) and sn_inflate_grid per map, sn_infer_batch per
pair, and the thing this stage replaces: a plain loop in C++ on one host thread over the same tables and map 0
(rollout_harness --bench), whose best sample and score must be the twin's.  The first three maps are compared with the numpy
twin's bytes before anything is timed.  Prints one JSON line; the gathers are counted from the samples' words (a sample that
collides stops at the end of its wave's 64-pair pass).

    python scripts/bench_rollout.py [--iters K] [--warmup W] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  first HIP-linked import (api.load_library)

from hobot_stereonet_amd import api, navfn, obstacles, rollout, synth, weights  # noqa: E402
from hobot_stereonet_amd.costmap import CostmapParams  # noqa: E402
from hobot_stereonet_amd.inflate import InflateParams  # noqa: E402
from hobot_stereonet_amd.navfn import NavParams  # noqa: E402
from hobot_stereonet_amd.obstacles import ObstacleParams  # noqa: E402
from hobot_stereonet_amd.pointcloud import Camera  # noqa: E402
from hobot_stereonet_amd.rollout import RolloutParams  # noqa: E402

W, H, D = 1280, 720, 192
N = 64
CAM = Camera(fx=1066.0, fy=1066.0, cx=639.5, cy=273.5, baseline_mm=120.0)
SCENE = ObstacleParams(base_from_cam=obstacles.mount(t=(0.0, 0.0, 0.5)), x_min_m=0.0, y_min_m=-5.0, cell_m=0.05, gw=200, gh=200, z_floor_m=-0.15,
                       z_lo_m=0.1, z_hi_m=1.5, beams=360, angle_min_rad=-0.54, angle_increment_rad=0.003, range_min_m=0.2, range_max_m=20.0)
MAP = CostmapParams(mw=400, mh=400, l_hit=85, l_miss=40, l_min=-200, l_max=350, clear_margin_m=0.1, clear_min_m=0.2, clear_max_m=0.0)
INFLATION = InflateParams(cell_m=0.05, inscribed_radius_m=0.2, inflation_radius_m=0.4, cost_scaling=10.0, lethal_min=50, flags=0)      # R = 8
PLAN = NavParams(neutral=50, lethal_cost=253, unknown_cost=20, flags=navfn.UNKNOWN_OK, max_rounds=0, max_path=1)
HARNESS = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat", "build", "rollout_harness")
ROLL = RolloutParams(cell_m=0.05, v_min=0.0, v_max=1.0, nv=21, w_min=-1.5, w_max=1.5, nw=41, sim_time_s=2.0, steps=20, lethal_cost=254,
                     centre_lethal_cost=253, unknown_cost=20, flags=rollout.UNKNOWN_OK, w_goal=1, w_occ=50)


def footprint():
    for spacing in (0.025, 0.05):
        try:
            return rollout.rectangle_footprint(0.6, 0.4, spacing), spacing
        except ValueError:
            pass
    raise SystemExit("no footprint fits")


def timed(call, st, warmup, iters):
    for _ in range(warmup):
        call()
    st.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters):
        call()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def gathers(samples, pairs):
    """cost bytes the kernel gathers for these samples: all pairs of a sample that does not collide, the passes of 64 pairs up to
    and with the one that holds the first colliding step's pairs otherwise (an upper bound: the first pair of that step), none
    outside the window"""
    reason = samples[..., 1] >> 8 & 0xff
    step = (samples[..., 1] >> 16).astype(np.int64)
    per_step = pairs // (ROLL.steps + 1)
    upto = np.minimum((step * per_step // rollout.WAVE + 1) * rollout.WAVE, pairs)
    return int(np.where(reason == rollout.COLLISION, upto, np.where(reason == rollout.OUT_OF_WINDOW, 0, pairs)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    fp, spacing = footprint()
    scene = np.stack([obstacles.ground_and_wall(W, H, CAM, 0.5, 6.0 - 0.05 * k) for k in range(N)])
    poses = np.stack([0.025 * np.arange(N), 0.4 * np.sin(np.arange(N) / 9.0), 0.3 * np.sin(np.arange(N) / 5.0)], axis=1)
    frames = np.stack([synth.sbs_nv12_frame(W, H, D, 21 + k).reshape(-1) for k in range(4)])
    gw, gh = MAP.mw, MAP.mh
    cells = gw * gh
    S, T1, pairs = ROLL.nv * ROLL.nw, ROLL.steps + 1, (ROLL.steps + 1) * (len(fp) + 1)
    rows = []
    with tempfile.TemporaryDirectory() as td:
        model = os.path.join(td, "m.snw")
        weights.save_snw(model, weights.synthetic(0), W, H, D)
        st = torch.cuda.Stream()
        with api.StereoNetHIP(model, max_batch=N) as eng:
            d_sbs = torch.from_numpy(np.ascontiguousarray(np.tile(frames, (N // 4, 1)))).cuda()
            dx = torch.empty((N, 6, H, W), dtype=torch.int8, device="cuda")
            d_net = torch.empty((N, H, W), dtype=torch.int32, device="cuda")
            eng.preprocess_sbs_nv12_device(N, d_sbs.data_ptr(), dx.data_ptr())
            torch.cuda.synchronize()
            fwd = {n: timed(lambda: eng.infer_device(n, dx.data_ptr(), d_net.data_ptr(), 0, st.cuda_stream), st, 3, 20) * 1e3 / n for n in (N, 1)}
            del dx, d_sbs, d_net
            d_raw = torch.from_numpy(scene).cuda()
            d_occ = torch.empty(N * SCENE.gw * SCENE.gh, dtype=torch.int8, device="cuda")
            d_rng = torch.empty(N * SCENE.beams, dtype=torch.float32, device="cuda")
            eng.obstacles_device(N, d_raw.data_ptr(), CAM, SCENE, occ_ptr=d_occ.data_ptr(), ranges_ptr=d_rng.data_ptr())
            d_map = torch.empty(N * cells, dtype=torch.int8, device="cuda")
            with eng.costmap(SCENE, MAP) as cm:      # the clip's 64 grids
                cm.push_device(N, poses, d_occ.data_ptr(), d_rng.data_ptr(), None, d_map.data_ptr(), 0, 0)
            d_cost = torch.empty(N * cells, dtype=torch.uint8, device="cuda")
            eng.inflate_device(N, d_map.data_ptr(), gw, gh, INFLATION, cost_ptr=d_cost.data_ptr())
            torch.cuda.synchronize()
            infl = {n: timed(lambda: eng.inflate_device(n, d_map.data_ptr(), gw, gh, INFLATION, cost_ptr=d_cost.data_ptr(), stream=st.cuda_stream),
                             st, args.warmup, args.iters) * 1e3 / n for n in (N, 1)}
            cost = d_cost.cpu().numpy().reshape(N, gh, gw)
            passable = navfn.weights(cost, PLAN) > 0
            goals = np.empty((N, 2), np.int32)
            for k in range(N):
                ys, xs = np.nonzero(passable[k])
                i = int(np.argmin((xs - (gw - 15)) ** 2 + (ys - gh // 2) ** 2))
                goals[k] = (xs[i], ys[i])
            d_goals = torch.from_numpy(goals).cuda()
            d_pot = torch.empty(N * cells, dtype=torch.int32, device="cuda")
            rounds = eng.navfn_device(N, d_cost.data_ptr(), gw, gh, d_goals.data_ptr(), 0, PLAN, potential_ptr=d_pot.data_ptr())
            fixed = NavParams(**{**PLAN.__dict__, "max_rounds": rounds + 1})
            nav = {n: timed(lambda: eng.navfn_device(n, d_cost.data_ptr(), gw, gh, d_goals.data_ptr(), 0, fixed, potential_ptr=d_pot.data_ptr(),
                                                     stream=st.cuda_stream), st, args.warmup, args.iters) * 1e3 / n for n in (N, 1)}
            eng.navfn_device(N, d_cost.data_ptr(), gw, gh, d_goals.data_ptr(), 0, PLAN, potential_ptr=d_pot.data_ptr())
            torch.cuda.synchronize()
            pot = d_pot.cpu().numpy().view(np.uint32).reshape(N, gh, gw)
            # the robot stands at the centre of its window and heads for the goal
            centre = ((gw // 2 + 0.5) * 0.05, (gh // 2 + 0.5) * 0.05)
            q = api.rollout_pose_q(ROLL.cell_m, 0.0, 0.0, [(centre[0], centre[1], float(np.arctan2((g[1] + 0.5) * 0.05 - centre[1], (g[0] + 0.5) * 0.05 - centre[0])))
                                                           for g in goals])
            d_q = torch.from_numpy(q).cuda()
            d_samples = torch.empty(N * S * 2, dtype=torch.int32, device="cuda")
            d_best = torch.empty(N * 8, dtype=torch.int32, device="cuda")
            d_traj = torch.zeros(N * T1 * 3, dtype=torch.int32, device="cuda")
            ptrs = (d_samples.data_ptr(), d_best.data_ptr(), d_traj.data_ptr())

            def call(n, out=ptrs, stream=0):
                eng.rollout_device(n, d_cost.data_ptr(), d_pot.data_ptr(), gw, gh, d_q.data_ptr(), ROLL, fp, 0, *out, stream=stream)

            tables = api.rollout_tables(ROLL, fp)
            want = rollout.reference(cost[:3], pot[:3], q[:3], None, ROLL, *tables)      # the twin's bytes before the clock starts
            call(3)
            torch.cuda.synchronize()
            if (d_samples[:3 * S * 2].cpu().numpy().view(np.uint32).tobytes() != want[0].tobytes()
                    or d_best[:24].cpu().numpy().view(np.uint32).tobytes() != want[1].tobytes()
                    or d_traj[:9 * T1].cpu().numpy().tobytes() != want[2].tobytes()):
                raise SystemExit("sn_rollout differs from the numpy twin")
            files = {"cost": cost[0], "pot": pot[0], "centres": tables[0], "offsets": tables[1]}
            for name, a in files.items():
                np.ascontiguousarray(a).tofile(os.path.join(td, name + ".bin"))
            host = json.loads(subprocess.run([HARNESS, "--bench"] + [os.path.join(td, k + ".bin") for k in files] +
                                             [str(v) for v in (gw, gh, ROLL.nv, ROLL.nw, ROLL.steps, len(fp), *q[0, :4].tolist(), ROLL.lethal_cost,
                                                               ROLL.centre_lethal_cost, ROLL.unknown_cost if ROLL.flags & rollout.UNKNOWN_OK else -1,
                                                               ROLL.w_goal, ROLL.w_occ, 20)], check=True, capture_output=True, text=True).stdout)
            if [host["s_best"], host["score"], host["valid"]] != [int(want[1][0, 1]), int(want[1][0, 2]) | int(want[1][0, 3]) << 32, int(want[1][0, 4])]:
                raise SystemExit(f"the host loop differs from the twin: {host} {want[1][0].tolist()}")
            call(N)
            torch.cuda.synchronize()
            samples = d_samples.cpu().numpy().view(np.uint32).reshape(N, S, 2)
            best = d_best.cpu().numpy().view(np.uint32).reshape(N, 8)
            for n in (N, 1):
                all_us = timed(lambda: call(n, stream=st.cuda_stream), st, args.warmup, args.iters) * 1e3
                best_us = timed(lambda: call(n, (0, ptrs[1], 0), st.cuda_stream), st, args.warmup, args.iters) * 1e3
                eval_us = timed(lambda: call(n, (ptrs[0], 0, 0), st.cuda_stream), st, args.warmup, args.iters) * 1e3
                g = gathers(samples[:n], pairs)
                rows.append({"n": n, "all_outputs_us": round(all_us, 2), "us_per_map": round(all_us / n, 3), "best_only_us": round(best_us, 2),
                             "samples_only_us": round(eval_us, 2), "second_launch_us": round(all_us - eval_us, 2),
                             "gathers": g, "gathers_full": n * S * pairs, "giga_gathers_per_s": round(g / eval_us / 1e3, 2),
                             "navfn_us_per_map": round(nav[n], 3), "inflate_us_per_map": round(infl[n], 3), "forward_us_per_pair": round(fwd[n], 3),
                             "fraction_of_forward": round(all_us / n / fwd[n], 5), "ratio_to_navfn": round(all_us / n / nav[n], 4),
                             "host_loop_us_per_map": host["loop_us"], "ratio_to_host_loop": round(all_us / n / host["loop_us"], 5),
                             "valid": int(best[:n, 4].sum()), "collided": int(best[:n, 5].sum()), "no_route": int(best[:n, 6].sum())})
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            # the same outline at the most points the contract takes (64, a spacing of 0.032 m), all outputs: how the time grows
            # towards the 80 points of a half-cell outline, which the call refuses
            fp64 = rollout.rectangle_footprint(0.6, 0.4, 0.032)
            want64 = rollout.reference(cost[:2], pot[:2], q[:2], None, ROLL, *api.rollout_tables(ROLL, fp64))
            dense = []

            def call64(n, stream=0):
                eng.rollout_device(n, d_cost.data_ptr(), d_pot.data_ptr(), gw, gh, d_q.data_ptr(), ROLL, fp64, 0, *ptrs, stream=stream)

            call64(2)
            torch.cuda.synchronize()
            if d_samples[:2 * S * 2].cpu().numpy().view(np.uint32).tobytes() != want64[0].tobytes() or d_best[:16].cpu().numpy().view(np.uint32).tobytes() != want64[1].tobytes():
                raise SystemExit("sn_rollout differs from the numpy twin at 64 points")
            for n in (N, 1):
                us = timed(lambda: call64(n, st.cuda_stream), st, args.warmup, args.iters) * 1e3
                dense.append({"n": n, "footprint_points": int(len(fp64)), "pairs_per_sample": T1 * (len(fp64) + 1), "all_outputs_us": round(us, 2),
                              "us_per_map": round(us / n, 3), "ratio_to_navfn": round(us / n / nav[n], 4)})
                print(json.dumps(dense[-1]), file=sys.stderr, flush=True)
            precision = api.PREC_NAMES.get(eng.precision_selected, "?")
    out = {"rollout_bench": True, "gpu": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "window": [gw, gh], "cell_m": 0.05,
           "samples": [ROLL.nv, ROLL.nw], "steps": ROLL.steps, "footprint_points": int(len(fp)), "footprint_spacing_m": spacing,
           "pairs_per_sample": pairs, "navfn_fixed_rounds": int(rounds + 1), "precision": precision, "host_loop": host,
           "params": {k: v for k, v in ROLL.__dict__.items() if k not in ("footprint", "pose", "acc")}, "rollout": rows, "rollout_64_points": dense}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
