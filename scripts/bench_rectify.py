#!/usr/bin/env python3
"""Times sn_rectify_nv12 (device buffers, a caller stream, device events, after warm-up) at batch 64 for raw pairs of 1280x720
and 1920x1080 rectified to the 1280x720 model, each writing the side-by-side frame alone and the frame plus the int8 tensor,
with sn_infer_batch per pair at the same batch on the same handle beside it.  The calibrations are rectify.synthetic_rig's
(barrel distortion, a few degrees between the eyes, zoom 0.8: about a fifth of the map is sentinels); the raw frames are
side-by-side NV12 of pitch 2 src_w.  Prints one JSON line.

    python scripts/bench_rectify.py [--iters K] [--warmup W] [--out FILE] [--ab-tree OTHER_CHECKOUT]

The stage is a gather: the floor is the bytes that must move per pair over the achievable HBM rate (6.3 TB/s, a float4 copy on
this part): the two maps once per CALL (2 * H * W * 8 bytes, shared by the call's pairs), both raw eyes once (2 * sw * sh * 3/2)
and the rectified frame once (3 * W * H).  `fraction_of_floor` = floor time / measured time of the frame-only call.

--ab-tree: a built checkout of another commit (the parent's) beside this one.  `bench.py --gpus 1 --steps 40 --warmup 5` is run
in child processes, this tree and the other in turn, twice each, and the four results are recorded in the order they ran: the
forward pass itself must not have changed.
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

from hobot_stereonet_amd import api, rectify, synth, weights  # noqa: E402

W, H, D, N = 1280, 720, 192, 64
SOURCES = [(1280, 720), (1920, 1080)]
HBM_BYTES_PER_S = 6.3e12


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


def forward_ms(eng, st, warmup, iters):
    seeds = np.stack([synth.model_input_i8(W, H, D, s) for s in range(4)])
    dx = torch.from_numpy(np.ascontiguousarray(np.tile(seeds, (N // 4, 1, 1, 1)))).cuda()
    raw = torch.empty((N, H, W), dtype=torch.int32, device="cuda")
    disp = torch.empty((N, H, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ms = timed(lambda: eng.infer_device(N, dx.data_ptr(), raw.data_ptr(), disp.data_ptr(), st.cuda_stream), st, warmup, iters)
    return {"n": N, "infer_batch_ms": round(ms, 4), "us_per_pair": round(ms * 1e3 / N, 3),
            "precision": api.PREC_NAMES.get(eng.precision_selected, "?")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--ab-tree", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    rows = []
    with tempfile.TemporaryDirectory() as td:
        model = os.path.join(td, "m.snw")
        weights.save_snw(model, weights.synthetic(0), W, H, D)
        with api.StereoNetHIP(model, max_batch=N) as eng:
            st = torch.cuda.Stream()
            fwd = forward_ms(eng, st, args.warmup, args.iters)
            sbs = torch.empty(N * 3 * W * H, dtype=torch.uint8, device="cuda")
            ten = torch.empty(N * 6 * W * H, dtype=torch.int8, device="cuda")
            for sw, sh in SOURCES:
                c = rectify.synthetic_rig(sw, sh, W, H, sw)
                frame = 2 * sw * (sh + sh // 2)
                src = torch.randint(0, 256, (N * frame,), dtype=torch.uint8, device="cuda")
                with eng.rectifier(c) as r:
                    info = r.info
                    torch.cuda.synchronize()
                    ms = {}
                    for tag, tp in (("frame", 0), ("frame_and_tensor", ten.data_ptr())):
                        ms[tag] = timed(lambda: r.rectify_device(N, src.data_ptr(), src.data_ptr() + sw, 2 * sw, frame, sbs.data_ptr(),
                                                                 tp, stream=st.cuda_stream), st, args.warmup, args.iters)
                floor_bytes = 2 * H * W * 8 / N + 2 * sw * sh * 3 // 2 + 3 * W * H
                floor_us = floor_bytes / HBM_BYTES_PER_S * 1e6
                us = ms["frame"] * 1e3 / N
                rows.append({"src": f"{sw}x{sh}", "n": N, "us_per_pair": round(us, 3),
                             "us_per_pair_with_tensor": round(ms["frame_and_tensor"] * 1e3 / N, 3),
                             "forward_us_per_pair": fwd["us_per_pair"], "share_of_forward": round(us / fwd["us_per_pair"], 4),
                             "valid_fraction": round((info["valid_left"] + info["valid_right"]) / (2.0 * W * H), 4),
                             "floor_bytes_per_pair": int(floor_bytes), "floor_us_per_pair": round(floor_us, 3),
                             "fraction_of_floor": round(floor_us / us, 4), "GB_per_s": round(floor_bytes / (us * 1e-6) / 1e9, 1)})
    out = {"rectify_bench": True, "width": W, "height": H, "dmax": D, "gpu": torch.cuda.get_device_name(0), "iters": args.iters,
           "warmup": args.warmup, "hbm_bytes_per_s": HBM_BYTES_PER_S, "forward": fwd, "rectify": rows}
    if args.ab_tree:      # fresh processes, after this one has let go of the GPU
        runs = []
        for tag, tree in (("this", ROOT), ("other", os.path.abspath(args.ab_tree))) * 2:
            env = {k: v for k, v in os.environ.items() if k != "STEREONET_HIP_LIB"}
            child = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "40", "--warmup", "5", "--no-cpu-baseline",
                                    "--no-end-to-end"], cwd=tree, env=env, capture_output=True, text=True, timeout=600)
            if child.returncode:
                raise SystemExit(f"--ab-tree: bench.py failed in {tree}:\n{child.stderr[-2000:]}")
            res = json.loads(child.stdout.strip().splitlines()[-1])
            runs.append({"tree": tag, "pairs_per_s": res.get("value"), "ms_per_step": res.get("ms_per_step"), "verified": res.get("verified")})
        mean = {t: float(np.mean([r["pairs_per_s"] for r in runs if r["tree"] == t])) for t in ("this", "other")}
        out["ab_bench_py"] = {"command": "bench.py --gpus 1 --steps 40 --warmup 5 --no-cpu-baseline --no-end-to-end", "runs": runs,
                              "this_over_other": round(mean["this"] / mean["other"], 4)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
