#!/usr/bin/env python3
"""Times sn_infer_conf beside sn_infer_batch and sn_infer_lrc (device buffers, a caller stream, device events, after warm-up)
at 1280x720 D=192, batch 64, default precision, on one handle:
    infer_batch        the plain forward, float + int32 maps (the yardstick), measured first and again last (drift)
    infer_conf         one forward + k_conf_apply: float map, confidence, mask and kept counts at min_conf 0.5
    infer_conf_plain   the same without a threshold: the plain maps plus the confidence
    infer_lrc          two forwards + the left-right check: float map, mask and kept counts
Prints one JSON line.

    python scripts/bench_conf.py [--iters K] [--warmup W] [--out FILE] [--batch-only]

--batch-only times infer_batch alone and touches no other entry point: run from a checkout of the parent commit it gives the
parent's figure on the same box.

What sn_infer_conf adds per pair: the soft-argmin epilogue writes one more 14 KB plane; k_conf_apply reads it and the 3.7 MB
int32 map and writes 3.7 MB of confidence, 0.9 MB of mask and 4 bytes of float map per rejected pixel (the int32 map is
rewritten only when the caller asks for it).
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

W, H, D, N = 1280, 720, 192, 64
TAU = (1.0, 0.0)
MIN_CONF = 0.5


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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--batch-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    seeds = np.stack([synth.model_input_i8(W, H, D, s) for s in range(4)])
    x = np.ascontiguousarray(np.tile(seeds, (N // 4, 1, 1, 1)))
    rows = []
    with tempfile.TemporaryDirectory() as td:
        model = os.path.join(td, "m.snw")
        weights.save_snw(model, weights.synthetic(0), W, H, D)
        with api.StereoNetHIP(model, max_batch=N) as eng:
            dx = torch.from_numpy(x).cuda()
            raw = torch.empty((N, H, W), dtype=torch.int32, device="cuda")
            disp = torch.empty((N, H, W), dtype=torch.float32, device="cuda")
            conf = torch.empty((N, H, W), dtype=torch.float32, device="cuda")
            mask = torch.empty((N, H, W), dtype=torch.uint8, device="cuda")
            kept = torch.empty(N, dtype=torch.int32, device="cuda")
            st = torch.cuda.Stream()
            s = st.cuda_stream
            torch.cuda.synchronize()
            calls = {"infer_batch": lambda: eng.infer_device(N, dx.data_ptr(), raw.data_ptr(), disp.data_ptr(), s)}
            if not args.batch_only:
                calls["infer_conf"] = lambda: eng.infer_conf_device(N, dx.data_ptr(), MIN_CONF, disp_ptr=disp.data_ptr(),
                                                                    conf_ptr=conf.data_ptr(), mask_ptr=mask.data_ptr(),
                                                                    kept_ptr=kept.data_ptr(), stream=s)
                calls["infer_conf_plain"] = lambda: eng.infer_conf_device(N, dx.data_ptr(), None, raw.data_ptr(), disp.data_ptr(),
                                                                          conf.data_ptr(), stream=s)
                calls["infer_lrc"] = lambda: eng.infer_lrc_device(N, dx.data_ptr(), TAU[0], TAU[1], disp_ptr=disp.data_ptr(),
                                                                  mask_ptr=mask.data_ptr(), kept_ptr=kept.data_ptr(), stream=s)
            calls["infer_batch_again"] = calls["infer_batch"]
            for name, call in calls.items():
                ms = timed(call, st, args.warmup, args.iters)
                row = {"call": name, "n": N, "ms": round(ms, 3), "pairs_per_s": round(N / (ms * 1e-3), 1)}
                if name in ("infer_conf", "infer_lrc"):
                    row["kept_fraction"] = round(float(kept.cpu().numpy().view(np.uint32).astype(np.int64).sum()) / (N * H * W), 4)
                rows.append(row)
            base = rows[0]["ms"]
            for row in rows:
                row["vs_infer_batch"] = round(row["ms"] / base, 4)
            precision = api.PREC_NAMES.get(eng.precision_selected, "?")
    line = json.dumps({"conf_bench": True, "width": W, "height": H, "dmax": D, "batch": N, "gpu": torch.cuda.get_device_name(0),
                       "precision": precision, "iters": args.iters, "warmup": args.warmup, "min_conf": MIN_CONF, "tau": TAU,
                       "batch_only": bool(args.batch_only), "rows": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
