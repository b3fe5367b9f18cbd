#!/usr/bin/env python3
"""Times the depth view (device buffers, a caller stream, device events, 50 calls after 5 warm-up) at 1280x720, batches 64 and 1,
on the engine's own maps of synth.sbs_nv12_frame pairs with the left eyes read in place from the side-by-side frames (pitch 2w):
sn_render into the NV12 and the RGB8 canvas, sn_render_jpeg (quality 95) with rows_per_slice 1 and 6; beside it sn_infer_batch per
pair at batch 64 on the same handle and the host path on one thread: RenderDepth + StackJoint (the colour map in double over
921 600 pixels and the stacked RGB canvas) and the host encoder EncodeNv12ToJpegSliced on the stacked 1280x1440 NV12 canvas.
Every GPU result is compared with the host C++ twin's bytes before it is timed.  Prints one JSON line.

    python scripts/bench_render.py [--iters K] [--warmup W] [--out FILE]

The byte floor per frame at the achievable HBM rate (6.3 TB/s, a float4 copy on this part), counted as scripts/bench_rectify.py
counts it, every byte that must move once: the map (4 W H), the left eye (1.5 W H) and the canvas (3 W H for NV12, 6 W H for
RGB8).  For sn_render_jpeg the canvas makes a round trip through the scratch (2 * 3 W H) and the encoder's own floor of
scripts/bench_jpeg.py follows (the coefficient round trip, three times the stream).  `fraction_of_floor` = floor time / measured.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  first HIP-linked import (api.load_library)

from hobot_stereonet_amd import api, render, synth, weights  # noqa: E402

W, H, D = 1280, 720, 192
HBM_BYTES_PER_S = 6.3e12
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")


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


def host_library():
    subprocess.check_call(["make", "-C", COMPAT, "-s"])
    lib = C.CDLL(os.path.join(COMPAT, "build", "libhobot_stereonet_node.so"))
    vp, ci = C.c_void_p, C.c_int
    lib.snhost_render.argtypes = [vp, C.c_long, ci, ci, vp, vp, vp, vp, vp]
    lib.snhost_render_canvas.argtypes = [ci, vp, vp, ci, ci, ci, vp, vp, ci, vp, ci, C.c_long]
    lib.snhost_jpeg_nv12_sliced.restype = C.c_long
    lib.snhost_jpeg_nv12_sliced.argtypes = [vp, ci, ci, ci, ci, ci, vp, C.c_long]
    return lib


def host_canvas(lib, raw, sbs, fmt):
    """RenderCanvas of one frame, reference parameters, minimal pitch"""
    rows, row_bytes = (3 * H, W) if fmt == render.NV12 else (2 * H, 3 * W)
    out = np.empty((rows, row_bytes), np.uint8)
    dp, ip = np.zeros(4, np.float64), np.zeros(4, np.int32)
    assert lib.snhost_render_canvas(1, raw.ctypes.data, sbs.ctypes.data, 2 * W, W, H, dp.ctypes.data, ip.ctypes.data, fmt,
                                    out.ctypes.data, row_bytes, rows * row_bytes) == 0
    return out


def host_path(lib, raw, sbs, canvas_nv12, rows, reps=3):
    """-> (ms of RenderDepth + StackJoint, ms of the encoder on the stacked canvas, the stream), one thread"""
    left_rgb = np.ascontiguousarray(render.nv12_to_rgb8(sbs, W, H, 2 * W)[0])
    payload = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    color, joint = np.empty((H, W, 3), np.uint8), np.empty((2 * H, W, 3), np.uint8)
    buf = np.empty(api.jpeg_bound(W, 2 * H), np.uint8)
    t0 = time.perf_counter()
    for _ in range(reps):
        assert lib.snhost_render(payload.ctypes.data, payload.size, W, H, None, None, color.ctypes.data, left_rgb.ctypes.data,
                                 joint.ctypes.data) == 4 * W * H
    t1 = time.perf_counter()
    for _ in range(reps):
        n = lib.snhost_jpeg_nv12_sliced(canvas_nv12.ctypes.data, W, 2 * H, W, 95, rows, buf.ctypes.data, buf.size)
    t2 = time.perf_counter()
    assert n > 0
    return (t1 - t0) * 1e3 / reps, (t2 - t1) * 1e3 / reps, buf[:n].tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    lib = host_library()
    N = 64
    frames = np.stack([synth.sbs_nv12_frame(W, H, D, 21 + k).reshape(-1) for k in range(4)])
    bound = api.jpeg_bound(W, 2 * H)
    blocks = ((W + 15) // 16) * ((2 * H + 15) // 16) * 6
    rows_out = []
    with tempfile.TemporaryDirectory() as td:
        model = os.path.join(td, "m.snw")
        weights.save_snw(model, weights.synthetic(0), W, H, D)
        with api.StereoNetHIP(model, max_batch=N) as eng:
            st = torch.cuda.Stream()
            d_sbs = torch.from_numpy(np.ascontiguousarray(np.tile(frames, (N // 4, 1)))).cuda()
            dx = torch.empty((N, 6, H, W), dtype=torch.int8, device="cuda")
            d_raw = torch.empty((N, H, W), dtype=torch.int32, device="cuda")
            eng.preprocess_sbs_nv12_device(N, d_sbs.data_ptr(), dx.data_ptr())
            torch.cuda.synchronize()
            fwd_ms = timed(lambda: eng.infer_device(N, dx.data_ptr(), d_raw.data_ptr(), 0, st.cuda_stream), st, 3, 20)
            fwd = {"n": N, "infer_batch_ms": round(fwd_ms, 4), "us_per_pair": round(fwd_ms * 1e3 / N, 3),
                   "precision": api.PREC_NAMES.get(eng.precision_selected, "?")}
            del dx
            raws = d_raw[:4].cpu().numpy()          # the engine's own maps of the four frames
            d_out = torch.empty(N * max(bound, 6 * H * W), dtype=torch.uint8, device="cuda")
            d_sz = torch.zeros(N, dtype=torch.int32, device="cuda")
            want = {fmt: [host_canvas(lib, raws[k], frames[k], fmt) for k in range(4)] for fmt in (render.NV12, render.RGB8)}
            host = {rows: [host_path(lib, raws[k], frames[k], want[render.NV12][k], rows) for k in range(4)] for rows in (1, 6)}
            left_floor = 4 * W * H + 1.5 * W * H
            for name, fmt, rows in (("render_nv12", render.NV12, 0), ("render_rgb8", render.RGB8, 0), ("render_jpeg", None, 1),
                                    ("render_jpeg", None, 6)):
                for n in (N, 1):
                    if fmt is not None:
                        row_bytes, nrows = (W, 3 * H) if fmt == render.NV12 else (3 * W, 2 * H)

                        def call():
                            eng.render_device(n, d_raw.data_ptr(), d_sbs.data_ptr(), 2 * W, None, fmt, d_out.data_ptr(), row_bytes,
                                              nrows * row_bytes, stream=st.cuda_stream)
                        call()
                        st.synchronize()
                        for k in range(min(n, 4)):       # the same bytes as the host twin, or the time means nothing
                            got = d_out[k * nrows * row_bytes:(k + 1) * nrows * row_bytes].cpu().numpy().reshape(nrows, row_bytes)
                            if not np.array_equal(got, want[fmt][k]):
                                raise SystemExit(f"{name} n {n}: frame {k} differs from the host twin")
                        floor_bytes = left_floor + nrows * row_bytes
                        extra = {}
                    else:
                        def call():
                            eng.render_jpeg_device(n, d_raw.data_ptr(), d_sbs.data_ptr(), 2 * W, None, 95, rows, d_out.data_ptr(), bound,
                                                   d_sz.data_ptr(), stream=st.cuda_stream)
                        call()
                        st.synchronize()
                        sizes = d_sz.cpu().numpy().view(np.uint32)[:n]
                        for k in range(min(n, 4)):
                            got = d_out[k * bound:k * bound + int(sizes[k])].cpu().numpy().tobytes()
                            if got != host[rows][k][2]:
                                raise SystemExit(f"{name} rows {rows} n {n}: frame {k} differs from the host encoder on the host canvas")
                        stream_bytes = float(np.mean([len(h[2]) for h in host[rows]]))
                        floor_bytes = left_floor + 2 * 3 * W * H + 2 * 128 * blocks + 3 * stream_bytes
                        extra = {"quality": 95, "rows_per_slice": rows, "stream_bytes_per_frame": int(stream_bytes),
                                 "host_encoder_ms_per_frame_and_thread": round(float(np.mean([h[1] for h in host[rows]])), 3)}
                    ms = timed(call, st, args.warmup, args.iters)
                    us = ms * 1e3 / n
                    floor_us = floor_bytes / HBM_BYTES_PER_S * 1e6
                    rows_out.append(dict({"call": name, "n": n, "us_per_frame": round(us, 3), "forward_us_per_pair": fwd["us_per_pair"],
                                          "share_of_forward": round(us / fwd["us_per_pair"], 4),
                                          "host_render_depth_stack_ms_per_frame": round(float(np.mean([h[0] for h in host[1]])), 3),
                                          "floor_bytes_per_frame": int(floor_bytes), "floor_us_per_frame": round(floor_us, 3),
                                          "fraction_of_floor": round(floor_us / us, 5),
                                          "GB_per_s": round(floor_bytes / (us * 1e-6) / 1e9, 1)}, **extra))
                    print(json.dumps(rows_out[-1]), file=sys.stderr, flush=True)
    out = {"render_bench": True, "width": W, "height": H, "gpu": torch.cuda.get_device_name(0), "iters": args.iters,
           "warmup": args.warmup, "hbm_bytes_per_s": HBM_BYTES_PER_S, "forward": fwd, "render": rows_out}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
