"""What the checkers themselves are worth: the C oracle (fp32) and the fp32 torch restatement against the float64 form
of the same restatement (torch_ref.truth) — the only thing in the tree more precise than what it judges.  Every
accuracy figure of the project used to be a distance from the fp32 oracle; DESIGN.md §3 now states them against this
truth, and tests/test_gpu_truth64.py holds every precision mode of the HIP path to it.  CPU only.

Bounds: mean <= 1e-4 px and max <= 1e-3 px for a checker's final map (the figure the round-6 verdict asked the oracle to
meet, and "no pixel of the checker is off by the whole budget"); every earlier stage below the same two numbers.  No
pixel is left out of any comparison."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from hobot_stereonet_amd import spec, synth, weights

CHECKER_MEAN, CHECKER_MAX = 1e-4, 1e-3
# name: (w, h, D, levels, weight seed, head gain, input seed)
CASES = {
    "c96x64_d48": (96, 64, 48, 1, 0, 1.0, 3), "c160x96_d96": (160, 96, 96, 1, 0, 1.0, 4), "c100x52_d32": (100, 52, 32, 1, 0, 1.0, 5),
    "c96x64_d48_multi": (96, 64, 48, spec.MULTI_LEVELS, 0, 1.0, 3), "c160x96_d96_multi": (160, 96, 96, spec.MULTI_LEVELS, 0, 1.0, 4),
    "c100x52_d32_multi": (100, 52, 32, spec.MULTI_LEVELS, 0, 1.0, 5),
    "c112x80_d64": (112, 80, 64, 1, 0, 1.0, 11),
    "C1_960x540_d48": (960, 540, 48, 1, 0, 1.0, 21),
    "C2_1280x720_d192": (1280, 720, 192, 1, 0, 1.0, 0),
    "C5_1242x375_d256_multi": (1242, 375, 256, spec.MULTI_LEVELS, 0, 1.0, 22),
}
_cache = {}


def _blob(seed, levels, gain):
    return weights.synthetic(seed, levels, head_gain=gain)


def _refs(oracle, name):
    import truth_compare as tc
    if name not in _cache:
        w, h, d, levels, ws, gain, si = CASES[name]
        _cache[name] = tc.Refs(oracle, _blob(ws, levels, gain), synth.model_input_i8(w, h, d, si), d)
    return _cache[name]


def test_float64_form_is_float64_all_the_way(monkeypatch, weights_multi):
    """dtype=torch.float64: every returned array is float64, the int8 input / 128 and the fp32 weights are widened exactly,
    and no convolution, pooling, interpolation, activation or softmax inside sees or returns anything narrower.  The
    default argument still returns float32 and the process-wide default dtype is untouched."""
    import torch_ref
    import truth_compare as tc
    seen = []

    def spy(mod, fn):
        orig = getattr(mod, fn)

        def wrapped(*a, **k):
            y = orig(*a, **k)
            seen.append((fn, [t.dtype for t in a if torch.is_tensor(t)] + [y.dtype]))
            return y
        monkeypatch.setattr(mod, fn, wrapped)

    for fn in ("conv2d", "conv3d", "interpolate", "avg_pool2d", "leaky_relu", "relu"):
        spy(torch_ref.F, fn)
    for fn in ("softmax", "cat", "zeros", "arange"):
        spy(torch_ref.torch, fn)
    w, h, d = 100, 52, 32
    x = synth.model_input_i8(w, h, d, 5)
    r = torch_ref.truth(weights_multi, x, d)
    tc.assert_float64(r)
    names = {fn for fn, _ in seen}
    assert {"conv2d", "conv3d", "interpolate", "avg_pool2d", "leaky_relu", "relu", "softmax", "cat", "zeros", "arange"} <= names
    for fn, dts in seen:
        assert all(dt == torch.float64 for dt in dts), (fn, dts)
    assert torch_ref._t(weights_multi, "ref2.res1.2.w", torch.float64).dtype == torch.float64
    assert np.array_equal(torch_ref._t(weights_multi, "agg.out.w", torch.float64).numpy(),
                          weights.tensor(weights_multi, "agg.out.w").astype(np.float64))
    assert len(r["levels"]) == spec.MULTI_LEVELS and r["disp"].shape == (h, w)
    seen.clear()
    r32 = torch_ref.forward(weights_multi, x, d)
    assert all(m.dtype == np.float32 for k, v in r32.items() for m in (v if k == "levels" else [v]))
    assert all(dt == torch.float32 for _, dts in seen for dt in dts)
    assert torch.get_default_dtype() == torch.float32


@pytest.mark.parametrize("name,w,h,d,seed", [("c96x64_d48", 96, 64, 48, 3), ("c160x96_d96", 160, 96, 96, 4), ("c100x52_d32", 100, 52, 32, 5)])
def test_default_dtype_still_produces_the_committed_goldens(oracle, golden_net, golden_multi, name, w, h, d, seed):
    """The committed goldens are fp32 runs of torch_ref.forward: threading the dtype through must not have moved them
    (conv kernels may differ between torch builds by summation order, hence 1e-4 px per pixel and not bit equality; on
    the build that wrote the goldens the arrays are identical)."""
    for g, key in ((golden_net, name), (golden_multi, name + "_multi")):
        r = _refs(oracle, key).t32
        assert np.abs(r["disp"] - g[name + ".disp"]).max() < 1e-4
        assert np.abs(r["disp_low"] - g[name + ".disp_low"]).max() < 1e-5
    assert np.abs(_refs(oracle, name).t32["cost"] - golden_net[name + ".cost"]).max() < 1e-4


def test_thread_pool_is_sized_by_the_environment(monkeypatch):
    import torch_ref
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    assert torch_ref.env_threads() == 3
    before = torch.get_num_threads()
    with torch_ref.torch_threads():
        assert torch.get_num_threads() == 3
    assert torch.get_num_threads() == before
    monkeypatch.delenv("OMP_NUM_THREADS")
    assert torch_ref.env_threads() == min(16, len(os.sched_getaffinity(0)))


@pytest.mark.parametrize("name", list(CASES))
def test_checkers_against_the_truth(oracle, name):
    """The C oracle and the fp32 torch run against the float64 truth: final map mean <= 1e-4 px, max <= 1e-3 px; disp_low,
    every coarse level map of the hierarchical model, the matching costs and both feature maps finite and below the same
    two numbers; the truth is not degenerate (differs from fp32, mean disparity > 1 px, no output pixel exactly zero — the
    final relu clips nothing on these inputs, and nothing would be masked if it did)."""
    import truth_compare as tc
    r = _refs(oracle, name)
    w, h, d, levels = CASES[name][:4]
    print(f"\n{name}: truth {r.seconds['truth']:.1f} s, torch fp32 {r.seconds['torch32']:.1f} s, oracle {r.seconds['oracle']:.1f} s")
    print(f"  final map     oracle E/M/signed {tc.fmt(r.e_oracle['disp'])}   torch fp32 {tc.fmt(r.e_t32['disp'])}")
    for k in r.e_t32:
        if k != "disp":
            o = tc.fmt(r.e_oracle[k][:2]) if k in r.e_oracle else "-"
            print(f"  {k:<13} oracle E/M {o:<20} torch fp32 {tc.fmt(r.e_t32[k][:2])}")
    tc.assert_float64(r.truth)
    assert r.truth["disp"].shape == (h, w) and sorted(r.levels) == list(range(1, levels))
    for who, e in (("oracle", r.e_oracle), ("torch fp32", r.e_t32)):
        assert e["disp"][0] <= CHECKER_MEAN and e["disp"][1] <= CHECKER_MAX, (who, e["disp"])
        for k, (em, mx, _) in e.items():
            assert np.isfinite([em, mx]).all() and em <= CHECKER_MEAN and mx <= CHECKER_MAX, (who, k, em, mx)
    assert levels == 1 or {"level1", "level2", "level3"} <= set(r.e_oracle)
    # not degenerate
    assert np.isfinite(r.truth["disp"]).all() and r.truth["disp"].mean() > 1.0
    assert (r.truth["disp"].astype(np.float32) != r.t32["disp"]).any() and (r.truth["cost"].astype(np.float32) != r.t32["cost"]).any()
    for m in (r.truth["disp"], r.t32["disp"], r.oracle["disp"]):
        assert int((m == 0).sum()) == 0
    assert r.oracle["raw"].min() >= 0


_CHILD = """
import hashlib, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/oracle"]
import oracle_py
from hobot_stereonet_amd import spec, synth, weights
for levels in (1, spec.MULTI_LEVELS):
    out = oracle_py.forward_levels(weights.synthetic(0, levels), synth.model_input_i8(160, 96, 96, 4), 96)
    h = hashlib.sha256()
    for a in (out[0], out[1], out[2], *out[3]):
        h.update(np.ascontiguousarray(a).tobytes())
    print(oracle_py.num_threads(), h.hexdigest())
"""


def test_oracle_does_not_depend_on_the_thread_count(oracle):
    """The oracle parallelises over output elements only (no reduction is split between threads), so its result is the same
    bit for bit with 1 and with many threads: E_ref measured where the GPU tests run equals E_ref measured anywhere."""
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    got = {}
    for n in ("1", "5"):
        env = dict(os.environ, OMP_NUM_THREADS=n)
        out = subprocess.run([sys.executable, "-c", _CHILD, root], env=env, check=True, capture_output=True, text=True, timeout=300).stdout
        lines = [ln.split() for ln in out.strip().splitlines()]
        assert [ln[0] for ln in lines] == [n, n], out
        got[n] = [ln[1] for ln in lines]
    assert got["1"] == got["5"]
    r = _refs(oracle, "c160x96_d96")                    # and the in-process run (whatever thread count it has) is that result too
    hs = hashlib.sha256()
    for a in (r.oracle["disp"], r.oracle["raw"], r.oracle["disp_low"]):
        hs.update(np.ascontiguousarray(a).tobytes())
    assert hs.hexdigest() == got["1"][0]


def _fp16_tower_weights(blob):
    """the same network with the 3x3 weights of its refinement tower rounded to fp16 (still computed in fp32 afterwards)"""
    out = blob.copy()
    for name, (off, shape) in spec.offsets(spec.levels_of(blob.size)).items():
        if name.startswith("ref") and name.endswith(".w") and ".res" in name:
            n = int(np.prod(shape))
            out[off:off + n] = out[off:off + n].astype(np.float16).astype(np.float32)
    return out


def test_the_comparison_can_fail(oracle):
    """The helper the GPU tests judge SN_PREC_FP32 with (truth_compare.fp32_class_failures, factor 3), fed at 1280x720 with
    maps that are wrong in ways the older bounds (mean vs oracle < 1e-3, per-pixel wire bound 0.02 px) let through:
    (a) fp32 torch map + 1e-2 px on one 60-column strip: mean +4.7e-4, over 3 E_ref only;
    (b) the same map + 5e-3 px on one column: caught by 3 M_ref only;
    (c) the fp32 torch map of the network with its tower's 3x3 weights rounded to fp16: a lost operand bit is coherent —
        caught by the signed mean (and narrowly by the mean).
    The unmodified fp32 torch map and the oracle's map pass."""
    import torch_ref
    import truth_compare as tc
    name = "C2_1280x720_d192"
    r = _refs(oracle, name)
    w, h, d, levels, ws, gain, si = CASES[name]
    truth, e_ref, m_ref = r.truth["disp"], r.E_ref, r.M_ref
    judge = lambda a: tc.fp32_class_failures(a, truth, e_ref, m_ref, tc.FP32_FACTOR)
    assert judge(r.t32["disp"]) == [] and judge(r.oracle["disp"]) == []
    a = r.t32["disp"].copy()
    a[:, 600:660] += 1e-2
    ea = tc.err(a, truth)
    assert ea[0] < 1e-3 and np.abs(a - r.oracle["disp"]).max() < 0.02          # what the older full-size bounds would see
    bad = judge(a)
    print(f"\n(a) strip:  E/M/signed {tc.fmt(ea)} vs 3 E_ref {3 * e_ref:.2e}, 3 M_ref {3 * m_ref:.2e}: {bad}")
    assert any(s.startswith("mean") for s in bad)
    b = r.t32["disp"].copy()
    b[:, 777] += 5e-3
    eb = tc.err(b, truth)
    bad = judge(b)
    print(f"(b) column: E/M/signed {tc.fmt(eb)}: {bad}")
    assert len(bad) == 1 and bad[0].startswith("max")
    with torch_ref.torch_threads():
        c = torch_ref.forward(_fp16_tower_weights(_blob(ws, levels, gain)), synth.model_input_i8(w, h, d, si), d)["disp"]
    ec = tc.err(c, truth)
    bad = judge(c)
    print(f"(c) fp16 tower weights in fp32 arithmetic: E/M/signed {tc.fmt(ec)} vs E_ref {e_ref:.2e}: {bad}")
    assert any(s.startswith("|signed mean|") for s in bad)
    assert ec[0] < 1e-3                                                        # ... and the budget alone would not notice
