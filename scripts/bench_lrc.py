#!/usr/bin/env python3
"""Times the left-right consistency check (device mode, device events, after warm-up) at 1280x720, D = 192, default precision,
device-resident input: sn_infer_lrc against sn_infer_batch on the same handle at n = 1, 16 and 64, and the two small kernels
alone at n = 64 on the maps of that inference.  Prints one JSON line.

    python scripts/bench_lrc.py [--iters K] [--warmup W] [--out FILE]

Algorithmic bytes per call (P = n * H * W pixels, J of them rejected):
    k_mirror_pair  12 * P              (6 int8 planes read, 6 written)
    k_lr_check     13 * P + 4 * J      (left and right map read, masked map and mask written, 0.0f stored at rejected pixels)
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  first HIP-linked import (api.load_library)

from hobot_stereonet_amd import api, synth, weights  # noqa: E402

W, H, D = 1280, 720, 192
HBM_BYTES_PER_S = 6.3e12      # the floor DESIGN §5g measures against
TAU = (1.0, 0.0)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    nmax = 64
    seeds = np.stack([synth.model_input_i8(W, H, D, s) for s in range(4)])
    x = np.ascontiguousarray(np.tile(seeds, (nmax // 4, 1, 1, 1)))
    composite, kernels = [], []
    with tempfile.TemporaryDirectory() as td:
        model = os.path.join(td, "m.snw")
        weights.save_snw(model, weights.synthetic(0), W, H, D)
        with api.StereoNetHIP(model, max_batch=nmax) as eng:
            dx = torch.from_numpy(x).cuda()
            raw = torch.empty((nmax, H, W), dtype=torch.int32, device="cuda")
            disp = torch.empty((nmax, H, W), dtype=torch.float32, device="cuda")
            right = torch.empty_like(raw)
            mask = torch.empty((nmax, H, W), dtype=torch.uint8, device="cuda")
            kept = torch.empty(nmax, dtype=torch.int32, device="cuda")
            st = torch.cuda.Stream()
            torch.cuda.synchronize()
            for n in (1, 16, 64):
                ms_fwd = timed(lambda: eng.infer_device(n, dx.data_ptr(), raw.data_ptr(), disp.data_ptr(), st.cuda_stream),
                               st, args.warmup, args.iters)
                ms_lrc = timed(lambda: eng.infer_lrc_device(n, dx.data_ptr(), TAU[0], TAU[1], raw.data_ptr(), disp.data_ptr(),
                                                            right.data_ptr(), mask.data_ptr(), kept.data_ptr(),
                                                            stream=st.cuda_stream), st, args.warmup, args.iters)
                k = kept[:n].cpu().numpy().view(np.uint32).astype(np.int64).sum()
                composite.append({"n": n, "infer_batch_ms": round(ms_fwd, 4), "infer_lrc_ms": round(ms_lrc, 4),
                                  "ratio": round(ms_lrc / ms_fwd, 4), "kept_fraction": round(float(k) / (n * H * W), 4),
                                  "precision": api.PREC_NAMES.get(eng.precision_selected, "?")})
            # the two kernels alone, n = 64: the left map unmasked, the second map as the network wrote it
            n = nmax
            mir = torch.empty_like(dx)
            second = torch.empty_like(raw)
            out = torch.empty_like(raw)
            eng.infer_device(n, dx.data_ptr(), raw.data_ptr(), disp.data_ptr(), st.cuda_stream)
            eng.mirror_pair_device(n, dx.data_ptr(), mir.data_ptr(), st.cuda_stream)
            eng.infer_device(n, mir.data_ptr(), second.data_ptr(), 0, st.cuda_stream)
            st.synchronize()
            px = n * H * W
            ms = timed(lambda: eng.mirror_pair_device(n, dx.data_ptr(), mir.data_ptr(), st.cuda_stream), st, args.warmup,
                       args.iters)
            kernels.append({"kernel": "k_mirror_pair", "n": n, "ms": round(ms, 4), "bytes": 12 * px})
            ms = timed(lambda: eng.lr_check_device(n, raw.data_ptr(), second.data_ptr(), TAU[0], TAU[1], True, out.data_ptr(),
                                                   disp.data_ptr(), mask.data_ptr(), kept.data_ptr(), st.cuda_stream),
                       st, args.warmup, args.iters)
            k = int(kept.cpu().numpy().view(np.uint32).astype(np.int64).sum())
            kernels.append({"kernel": "k_lr_check", "n": n, "ms": round(ms, 4), "bytes": 13 * px + 4 * (px - k),
                            "kept_fraction": round(k / px, 4)})
            for r in kernels:
                r["GB_per_s"] = round(r["bytes"] / (r["ms"] * 1e-3) / 1e9, 1)
                r["share_of_floor"] = round(r["bytes"] / HBM_BYTES_PER_S / (r["ms"] * 1e-3), 3)
    line = json.dumps({"lrc_bench": True, "width": W, "height": H, "dmax": D, "gpu": torch.cuda.get_device_name(0),
                       "iters": args.iters, "warmup": args.warmup, "tau": TAU, "composite": composite, "kernels": kernels})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
