"""The C-ABI library builds, loads without a GPU, exports every symbol include/stereonet_hip.h declares,
and fails loudly (never falls back to a CPU path) when no gfx950 device is present."""
import ctypes
import os
import re

import pytest

from hobot_stereonet_amd import api, build, weights

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "stereonet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sn_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_exported():
    lib = ctypes.CDLL(build.build())
    syms = declared_symbols()
    assert len(syms) >= 15
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in stereonet_hip.h but not exported"


def declared_parameter_counts():
    """name -> number of parameters of every sn_* prototype in the header (commas at depth 0 of its parameter list)"""
    src = open(os.path.join(ROOT, "include", "stereonet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    counts = {}
    for m in re.finditer(r"\b(sn_[a-z0-9_]+)\s*\(", src):
        depth, commas, i = 1, 0, m.end()
        while depth:
            c = src[i]
            depth += (c == "(") - (c == ")")
            commas += c == "," and depth == 1
            i += 1
        params = src[m.end():i - 1].strip()
        counts[m.group(1)] = 0 if params in ("", "void") else commas + 1
    return counts


def test_bound_argtypes_have_the_headers_parameter_counts():
    """api.py writes every argtypes list by hand: each declared function has one, as long as its prototype's parameter list
    (a hook that gained a parameter would otherwise still be called with the old arguments).  Only a function without
    parameters may go without a list (sn_abi_version)."""
    lib = api.load_library()
    counts = declared_parameter_counts()
    assert len([s for s in counts if s.startswith("sn_dbg_")]) >= 20 and sorted(counts) == declared_symbols()
    for name, n in counts.items():
        argtypes = getattr(lib, name).argtypes
        assert argtypes is not None or (n == 0 and not name.startswith("sn_dbg_")), f"{name}: api.py sets no argtypes"
        assert len(argtypes or ()) == n, f"{name}: {len(argtypes or ())} argtypes bound, {n} parameters declared"


def test_slot_graph_readout_is_exported_and_refuses_null():
    """sn_dbg_slot_graphs (what the async slots' hipGraphs did; tests/test_gpu_async_graph.py) is a test hook: exported and
    bound by api.py, not declared in the public header, and SN_ERR_ARG for a null handle or a null output without a device."""
    lib = api.load_library()
    assert hasattr(lib, "sn_dbg_slot_graphs") and hasattr(api.StereoNetHIP, "dbg_slot_graphs")
    assert "sn_dbg_slot_graphs" not in declared_symbols()
    a, b, c = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_int(7)
    assert lib.sn_dbg_slot_graphs(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == -1      # SN_ERR_ARG
    assert (a.value, b.value, c.value) == (7, 7, 7)             # nothing written


def test_strerror_and_codes():
    assert api.error_string(0) == "ok"
    assert "gfx950" in api.error_string(-4)
    assert "65504" in api.error_string(-8)      # SN_ERR_RANGE
    assert api.error_string(-99) == "unknown error"


def test_create_without_gpu_fails_loudly(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = str(tmp_path / "m.snw")
    weights.save_snw(p, weights.synthetic(0))
    with pytest.raises(api.StereoNetError) as e:
        api.StereoNetHIP(p)
    assert e.value.code == -4        # SN_ERR_DEVICE: no silent CPU path


def test_product_does_not_touch_oracle():
    # the oracle is test infrastructure: nothing under hobot_stereonet_amd/ may reference it
    for dirpath, _, files in os.walk(os.path.join(ROOT, "hobot_stereonet_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle_py" not in txt and "libstereonet_oracle" not in txt and "so_forward" not in txt, f
