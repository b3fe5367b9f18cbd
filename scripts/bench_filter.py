#!/usr/bin/env python3
"""Times sn_filter_raw (device buffers, a caller stream, device events, after warm-up) at 1280x720 for n = 1, 16 and 64 on
four inputs, with sn_infer_batch per map at the same n on the same handle beside it (the forward is the yardstick):
    lrc       the masked output of sn_infer_lrc on synth pairs            speckle 200 px / 1 px, fill 16
    constant  one component of H*W pixels                                 the same
    noise     30 % zeros, random values: about half a million components  the same
    fill      the lrc maps, fill 16 only (one kernel)
Every call writes out_raw (not in place), the mask, the float map and the counts.  Prints one JSON line.

    python scripts/bench_filter.py [--iters K] [--warmup W] [--out FILE]

First-touch bytes per call (P = n * H * W pixels, J of them with a mask other than 0; the root gathers label[label[p]] and
size[root] stay in the caches and are not counted):
    k_flt_label    12 * P      raw read, label and size written
    k_flt_seam     <= 1.25 * P  two (four) raw values per border pair, 1/64 + 1/16 pairs per pixel; its atomics are few
    k_flt_flatten   4 * P      size read (label and size touched at tile roots only)
    k_flt_apply    13 * P + 4 * J with speckle removal (raw, label read; out_raw, mask written; the float map at J pixels),
                    9 * P + 4 * J for the fill alone
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  first HIP-linked import (api.load_library)

from hobot_stereonet_amd import api, synth, weights  # noqa: E402

W, H, D = 1280, 720, 192
HBM_BYTES_PER_S = 6.3e12      # the floor DESIGN §5g measures against
TAU = (1.0, 0.0)
BOTH, FILL = (200, 1.0, 16), (0, 1.0, 16)


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    nmax = 64
    seeds = np.stack([synth.model_input_i8(W, H, D, s) for s in range(4)])
    x = np.ascontiguousarray(np.tile(seeds, (nmax // 4, 1, 1, 1)))
    rng = np.random.default_rng(0)
    noise = rng.integers(1, 50000, (4, H, W)).astype(np.int32)
    noise[rng.random(noise.shape) < 0.3] = 0
    rows, forward = [], []
    with tempfile.TemporaryDirectory() as td:
        model = os.path.join(td, "m.snw")
        weights.save_snw(model, weights.synthetic(0), W, H, D)
        with api.StereoNetHIP(model, max_batch=nmax) as eng:
            dx = torch.from_numpy(x).cuda()
            lrc = torch.empty((nmax, H, W), dtype=torch.int32, device="cuda")
            disp = torch.empty((nmax, H, W), dtype=torch.float32, device="cuda")
            out = torch.empty_like(lrc)
            mask = torch.empty((nmax, H, W), dtype=torch.uint8, device="cuda")
            counts = torch.empty((nmax, 3), dtype=torch.int32, device="cuda")
            st = torch.cuda.Stream()
            torch.cuda.synchronize()
            fwd_ms = {}
            for n in (1, 16, 64):
                fwd_ms[n] = timed(lambda: eng.infer_device(n, dx.data_ptr(), out.data_ptr(), disp.data_ptr(), st.cuda_stream),
                                  st, args.warmup, args.iters)
                forward.append({"n": n, "infer_batch_ms": round(fwd_ms[n], 4), "ms_per_map": round(fwd_ms[n] / n, 4),
                                "precision": api.PREC_NAMES.get(eng.precision_selected, "?")})
            eng.infer_lrc_device(nmax, dx.data_ptr(), TAU[0], TAU[1], lrc.data_ptr(), disp.data_ptr(), stream=st.cuda_stream)
            st.synchronize()
            inputs = {"lrc": (lrc, BOTH), "constant": (torch.full_like(lrc, 66000), BOTH),
                      "noise": (torch.from_numpy(np.ascontiguousarray(np.tile(noise, (nmax // 4, 1, 1)))).cuda(), BOTH),
                      "fill": (lrc, FILL)}
            torch.cuda.synchronize()
            for name, (src, params) in inputs.items():
                for n in (1, 16, 64):
                    def call(stream=st.cuda_stream):
                        eng.filter_raw_device(n, src.data_ptr(), *params, out_raw_ptr=out.data_ptr(), mask_ptr=mask.data_ptr(),
                                              disp_ptr=disp.data_ptr(), counts_ptr=counts.data_ptr(), stream=stream)
                    ms = timed(call, st, args.warmup, args.iters)
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        call(0)                                  # the filter's own stream: returns after completion
                    wall = (time.perf_counter() - t0) * 1e3 / args.iters
                    c = counts[:n].cpu().numpy().view(np.uint32).astype(np.int64).sum(0)
                    px = n * H * W
                    touched = int((mask[:n] != 0).sum().item())
                    nbytes = (29 if params[0] else 9) * px + 4 * touched
                    rows.append({"input": name, "n": n, "params": params, "ms": round(ms, 4), "ms_per_map": round(ms / n, 4),
                                 "own_stream_wall_ms_per_map": round(wall / n, 4),
                                 "forward_ms_per_map": round(fwd_ms[n] / n, 4), "share_of_forward": round(ms / fwd_ms[n], 4),
                                 "valid_fraction": round(float(c[0]) / px, 4), "removed": int(c[1]), "filled": int(c[2]),
                                 "bytes": nbytes, "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                                 "share_of_floor": round(nbytes / HBM_BYTES_PER_S / (ms * 1e-3), 3)})
    line = json.dumps({"filter_bench": True, "width": W, "height": H, "dmax": D, "gpu": torch.cuda.get_device_name(0),
                       "iters": args.iters, "warmup": args.warmup, "tau": TAU, "forward": forward, "filter": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
