#!/usr/bin/env python3
"""Times sn_temporal_push (device buffers, a caller stream, device events, after warm-up) at 1280x720 for one stream x 16
frames, 64 streams x 1 frame and n = 1, each GUIDED (luma_delta 24 with the int8 model input as the guide, and the float map
patched) and PLAIN (luma_delta 0: no guide, no float map).  Every call writes out_raw (not in place), the mask and the counts.
In the same run and on the same handle: sn_infer_batch per map at the same n (the yardstick of the other stages: a setting that
costs more per map than the forward at batch 64 counts as unfinished), and a device-to-device hipMemcpyAsync that moves the
same number of bytes as the kernel (the memory-bound yardstick; a copy of B / 2 bytes reads B / 2 and writes B / 2).
Prints one JSON line.

    python scripts/bench_temporal.py [--iters K] [--warmup W] [--out FILE]

The kernel has no neighbourhood: per pixel and frame it reads raw 4 (+ luma 1) and writes out 4 + mask 1 (+ 4 where the float
map changes), and per pixel, stream and launch it reads and writes the state once (P 4 + Hs 1, + Yp 1 when guided).
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  first HIP-linked import (api.load_library)

from hobot_stereonet_amd import api, synth, temporal, weights  # noqa: E402

W, H, D = 1280, 720, 192
PARAMS = {"guided": (64, 0.5, 2, 24), "plain": (64, 0.5, 2, 0)}
CASES = [("1 stream x 16 frames", 16, None), ("64 streams x 1 frame", 64, list(range(64))), ("n = 1", 1, None)]


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


def hip_runtime():
    """The HIP runtime this process has loaded already (torch's copy, or the system's): the copy must not bring a second one."""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    return C.CDLL("libamdhip64.so")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    nmax = 64
    clip, luma, _ = temporal.noisy_sequence(W, H, 16, 1)
    maps = np.ascontiguousarray(np.tile(clip, (nmax // 16, 1, 1)))
    seeds = np.stack([synth.model_input_i8(W, H, D, s) for s in range(4)])
    x = np.ascontiguousarray(np.tile(seeds, (nmax // 4, 1, 1, 1)))
    x[:, 0] = (np.tile(luma, (nmax // 16, 1, 1)) ^ np.uint8(0x80)).view(np.int8)      # channel 0 carries the clip's luma
    rows, forward = [], []
    with tempfile.TemporaryDirectory() as td:
        model = os.path.join(td, "m.snw")
        weights.save_snw(model, weights.synthetic(0), W, H, D)
        with api.StereoNetHIP(model, max_batch=nmax) as eng:
            dx = torch.from_numpy(x).cuda()
            raw = torch.from_numpy(maps).cuda()
            disp0 = torch.from_numpy((maps.astype(np.float32) * temporal.wire_scale(eng.out_scale))).cuda()
            disp = disp0.clone()
            out = torch.empty_like(raw)
            mask = torch.empty((nmax, H, W), dtype=torch.uint8, device="cuda")
            counts = torch.empty((nmax, 4), dtype=torch.int32, device="cuda")
            src = torch.empty(nmax * H * W * 14, dtype=torch.uint8, device="cuda")      # the largest case moves 13 bytes per pixel and way
            dst = torch.empty_like(src)
            st = torch.cuda.Stream()
            torch.cuda.synchronize()
            fwd_ms = {}
            for n in (1, 16, 64):
                fwd_ms[n] = timed(lambda: eng.infer_device(n, dx.data_ptr(), out.data_ptr(), disp.data_ptr(), st.cuda_stream),
                                  st, args.warmup, args.iters)
                forward.append({"n": n, "infer_batch_ms": round(fwd_ms[n], 4), "us_per_map": round(fwd_ms[n] / n * 1e3, 2),
                                "precision": api.PREC_NAMES.get(eng.precision_selected, "?")})
            for name, n, ids in CASES:
                for kind, prm in PARAMS.items():
                    guided = prm[3] > 0
                    streams = n if ids else 1
                    with eng.temporal_filter(streams, *prm) as tf:
                        def call():
                            tf.push_device(n, raw.data_ptr(), dx.data_ptr() if guided else 0, api.SN_GUIDE_TENSOR, 0, stream_of=ids,
                                           out_raw_ptr=out.data_ptr(), mask_ptr=mask.data_ptr(),
                                           disp_ptr=disp.data_ptr() if guided else 0, counts_ptr=counts.data_ptr(),
                                           stream=st.cuda_stream)
                        disp.copy_(disp0)
                        torch.cuda.synchronize()
                        ms = timed(call, st, args.warmup, args.iters)
                        c = counts[:n].cpu().numpy().view(np.uint32).astype(np.int64).sum(0)
                        changed = int((out[:n] != torch.clamp(raw[:n], min=0)).sum().item())
                    px = n * H * W
                    state = 2 * (6 if guided else 5) * streams * H * W          # read and written once per launch and stream
                    nbytes = (10 if guided else 9) * px + (4 * changed if guided else 0) + state
                    copy_bytes = nbytes // 2 // 16 * 16
                    assert copy_bytes <= src.numel()

                    def copy():
                        hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), copy_bytes, 3, st.cuda_stream)      # device to device
                    copy_ms = timed(copy, st, args.warmup, args.iters)
                    rows.append({"case": name, "setting": kind, "params": list(prm), "n": n, "streams": streams,
                                 "us": round(ms * 1e3, 2), "us_per_map": round(ms / n * 1e3, 2),
                                 "forward_us_per_map": round(fwd_ms[n] / n * 1e3, 2),
                                 "share_of_forward_at_64": round((ms / n) / (fwd_ms[64] / 64), 4),
                                 "valid": int(c[0]), "blended": int(c[1]), "held": int(c[2]), "moved_or_jump": int(c[3]),
                                 "changed": changed, "bytes": nbytes, "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                                 "copy_bytes": copy_bytes, "copy_us": round(copy_ms * 1e3, 2),
                                 "copy_GB_per_s": round(2 * copy_bytes / (copy_ms * 1e-3) / 1e9, 1),
                                 "ratio_to_copy": round(ms / copy_ms, 3)})
    line = json.dumps({"temporal_bench": True, "width": W, "height": H, "dmax": D, "gpu": torch.cuda.get_device_name(0),
                       "iters": args.iters, "warmup": args.warmup, "forward": forward, "temporal": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
