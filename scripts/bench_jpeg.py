#!/usr/bin/env python3
"""Times sn_jpeg_encode_nv12 (device buffers, a caller stream, device events, 50 calls after 5 warm-up) on 1280x720 left eyes read
in place from side-by-side frames (pitch 2w): synth.sbs_nv12_frame content and white noise (the entropy coder's worst case),
batches 1 and 64, qualities 75 and 95, rows_per_slice 1 and 6, with sn_infer_batch per pair at batch 64 on the same handle and
the host encoder (EncodeNv12ToJpegSliced, one thread, the same frames) beside it.  Every GPU stream is compared with the host
encoder's before it is timed.  Prints one JSON line.

    python scripts/bench_jpeg.py [--iters K] [--warmup W] [--out FILE]

The byte floor per frame at the achievable HBM rate (6.3 TB/s, a float4 copy on this part): the image read once (1.5 W H) and
the stream written once, plus -- the kernels are not fused -- the coefficient round trip (2 * 128 bytes per block) and the
slices' round trip through the scratch (2 * stream).  `fraction_of_floor` = floor time / measured time.
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

from hobot_stereonet_amd import api, synth, weights  # noqa: E402

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
    lib.snhost_jpeg_nv12_sliced.restype = C.c_long
    lib.snhost_jpeg_nv12_sliced.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long]
    return lib


def host_encode(lib, frame, quality, rows, buf, reps=1):
    """-> (stream, ms per frame on one thread)"""
    t0 = time.perf_counter()
    for _ in range(reps):
        n = lib.snhost_jpeg_nv12_sliced(frame.ctypes.data, W, H, 2 * W, quality, rows, buf.ctypes.data, buf.size)
    ms = (time.perf_counter() - t0) * 1e3 / reps
    assert n > 0
    return buf[:n].tobytes(), ms


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
    rng = np.random.default_rng(5)
    contents = {"synth": np.stack([synth.sbs_nv12_frame(W, H, D, 21 + k).reshape(-1) for k in range(4)]),
                "noise": rng.integers(0, 256, (4, 3 * W * H), dtype=np.uint8)}
    bound = api.jpeg_bound(W, H)
    hbuf = np.empty(bound, np.uint8)
    blocks = ((W + 15) // 16) * ((H + 15) // 16) * 6
    rows_out = []
    with tempfile.TemporaryDirectory() as td:
        model = os.path.join(td, "m.snw")
        weights.save_snw(model, weights.synthetic(0), W, H, D)
        with api.StereoNetHIP(model, max_batch=N) as eng:
            st = torch.cuda.Stream()
            seeds = np.stack([synth.model_input_i8(W, H, D, s) for s in range(4)])
            dx = torch.from_numpy(np.ascontiguousarray(np.tile(seeds, (N // 4, 1, 1, 1)))).cuda()
            raw = torch.empty((N, H, W), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            fwd_ms = timed(lambda: eng.infer_device(N, dx.data_ptr(), raw.data_ptr(), 0, st.cuda_stream), st, 3, 20)
            fwd = {"n": N, "infer_batch_ms": round(fwd_ms, 4), "us_per_pair": round(fwd_ms * 1e3 / N, 3),
                   "precision": api.PREC_NAMES.get(eng.precision_selected, "?")}
            del dx, raw
            d_out = torch.empty(N * bound, dtype=torch.uint8, device="cuda")
            d_sz = torch.zeros(N, dtype=torch.int32, device="cuda")
            for name, four in contents.items():
                d_in = torch.from_numpy(np.ascontiguousarray(np.tile(four, (N // 4, 1)))).cuda()
                for quality in (75, 95):
                    for rows in (1, 6):
                        want, host_ms = zip(*(host_encode(lib, four[k], quality, rows, hbuf, 3) for k in range(4)))
                        for n in (1, N):
                            def call():
                                eng.jpeg_encode_nv12_device(n, d_in.data_ptr(), W, H, 2 * W, 3 * W * H, quality, rows, d_out.data_ptr(),
                                                            bound, d_sz.data_ptr(), stream=st.cuda_stream)
                            call()
                            st.synchronize()
                            sizes = d_sz.cpu().numpy().view(np.uint32)[:n]
                            for k in range(min(n, 4)):       # the same bytes as the host encoder, or the time means nothing
                                got = d_out[k * bound:k * bound + int(sizes[k])].cpu().numpy().tobytes()
                                if got != want[k]:
                                    raise SystemExit(f"{name} q{quality} rows {rows} n {n}: frame {k} differs from the host encoder")
                            ms = timed(call, st, args.warmup, args.iters)
                            stream_bytes = float(np.mean([len(s) for s in want]))
                            floor_bytes = 1.5 * W * H + stream_bytes + 2 * 128 * blocks + 2 * stream_bytes
                            us = ms * 1e3 / n
                            rows_out.append({"content": name, "quality": quality, "rows_per_slice": rows, "n": n,
                                             "us_per_frame": round(us, 3), "stream_bytes_per_frame": int(stream_bytes),
                                             "host_ms_per_frame_and_thread": round(float(np.mean(host_ms)), 3),
                                             "forward_us_per_pair": fwd["us_per_pair"],
                                             "share_of_forward": round(us / fwd["us_per_pair"], 4),
                                             "floor_bytes_per_frame": int(floor_bytes),
                                             "floor_us_per_frame": round(floor_bytes / HBM_BYTES_PER_S * 1e6, 3),
                                             "fraction_of_floor": round(floor_bytes / HBM_BYTES_PER_S * 1e6 / us, 5)})
                            print(json.dumps(rows_out[-1]), file=sys.stderr, flush=True)
                del d_in
    out = {"jpeg_bench": True, "width": W, "height": H, "gpu": torch.cuda.get_device_name(0), "iters": args.iters,
           "warmup": args.warmup, "hbm_bytes_per_s": HBM_BYTES_PER_S, "fused": False, "forward": fwd, "jpeg": rows_out}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
