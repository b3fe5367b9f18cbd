"""The JPEG encoder's contract on the CPU: the numpy twin (hobot_stereonet_amd/jpeg.py) equals the host C++ encoder
(EncodeNv12ToJpegSliced, through the compat library's hooks) byte for byte over sizes, qualities, restart intervals and pitches;
every stream decodes; sliced and single-scan streams decode to the same pixels; the inputs exercise what the GPU tests
(tests/test_gpu_jpeg.py) rely on (stuffing, ZRL, blocks without EOB, the extreme DC categories, large AC categories, RSTm
wrap-around, edge replication); rounding ties go to even; the Python binding agrees with the header.

No tolerance appears: the arithmetic is float32 operation by operation on both sides, and entropy coding is in integers."""
import ctypes as C
import functools
import io
import os
import re
import subprocess

import numpy as np
import pytest

from hobot_stereonet_amd import api, jpeg

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
HEADER = open(os.path.join(ROOT, "include", "stereonet_hip.h")).read()

SIZES = ((96, 64), (70, 50), (34, 18), (132, 70), (48, 160), (2, 2))
QUALITIES = (1, 50, 75, 95, 100)
ROWS = (0, 1, 3, 99)
KINDS = ("noise", "bands", "hf", "checker", "stripes")


def pitches(w):
    return (w, 2 * w, w + 6)


@functools.lru_cache(maxsize=None)
def host_library():
    from hobot_stereonet_amd import build
    build.build()
    subprocess.check_call(["make", "-C", COMPAT, "-s"])
    import torch  # noqa: F401  (before anything that links HIP: one HIP runtime per process, see api.load_library)
    lib = C.CDLL(os.path.join(COMPAT, "build", "libhobot_stereonet_node.so"))
    vp, ci = C.c_void_p, C.c_int
    lib.snhost_jpeg_nv12.restype = C.c_long
    lib.snhost_jpeg_nv12.argtypes = [vp, ci, ci, ci, ci, vp, C.c_long]
    lib.snhost_jpeg_nv12_sliced.restype = C.c_long
    lib.snhost_jpeg_nv12_sliced.argtypes = [vp, ci, ci, ci, ci, ci, vp, C.c_long]
    return lib


def host_encode(img, w, h, pitch, quality, rows_per_slice) -> bytes:
    """EncodeNv12ToJpegSliced of the compat library"""
    lib = host_library()
    src = np.ascontiguousarray(img, np.uint8).reshape(-1)
    buf = np.empty(api.jpeg_bound(w, h), np.uint8)
    n = lib.snhost_jpeg_nv12_sliced(src.ctypes.data, w, h, pitch, quality, rows_per_slice, buf.ctypes.data, buf.size)
    assert n > 0
    return buf[:n].tobytes()


def decode(stream: bytes) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))


def matrix():
    """(kind, w, h, pitch, quality, rows_per_slice) of the whole product; the content cycles through KINDS"""
    i = 0
    for w, h in SIZES:
        for q in QUALITIES:
            for r in ROWS:
                for p in pitches(w):
                    yield KINDS[i % len(KINDS)], w, h, p, q, r
                    i += 1


@functools.lru_cache(maxsize=None)
def twin_case(kind, w, h, pitch, quality, rows_per_slice, seed=0):
    """-> (image, the twin's stream, its stats), computed once"""
    img = jpeg.sample_image(kind, w, h, pitch, seed + w + quality)
    img.setflags(write=False)
    stream, st = jpeg._encode(img, w, h, pitch, quality, rows_per_slice)
    return img, stream, st


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_twin_equals_host_encoder_byte_for_byte(w, h):
    bad = []
    for kind, cw, ch, p, q, r in matrix():
        if (cw, ch) != (w, h):
            continue
        img, stream, st = twin_case(kind, cw, ch, p, q, r)
        want = host_encode(img, w, h, p, q, r)
        restart = jpeg.restart_mcus(w, h, r)
        assert stream[:2] == b"\xff\xd8" and stream[-2:] == b"\xff\xd9"
        assert (stream.count(b"\xff\xdd\x00\x04") >= 1) == (restart > 0)
        assert stream[:jpeg.HEADER_BYTES + (6 if restart else 0)] == jpeg.header(w, h, q, restart)
        assert len(stream) <= api.jpeg_bound(w, h)
        if stream != want:
            bad.append((kind, p, q, r, len(stream), len(want)))
        px = decode(stream)                                      # every stream decodes to the size given
        assert px.shape == (h, w, 3), (kind, p, q, r)
        if r:                                                    # ... and to the pixels of the single scan
            single = twin_case(kind, w, h, p, q, 0)[1]
            assert np.array_equal(px, decode(single)), (kind, p, q, r)
    assert not bad, bad


def test_twin_equals_host_encoder_at_full_size():
    w, h = 1280, 720
    img = jpeg.sample_image("bands", w, h, w, 3)
    stream = jpeg.encode_nv12(img, w, h, w, 95, 6)
    assert stream == host_encode(img, w, h, w, 95, 6)
    assert decode(stream).shape == (h, w, 3)


def test_quality_is_clamped_and_sizes_are_checked():
    w, h = 34, 18
    img = jpeg.sample_image("bands", w, h, w, 1)
    for q, same in ((0, 1), (-7, 1), (101, 100), (1000, 100)):
        assert jpeg.encode_nv12(img, w, h, w, q, 1) == jpeg.encode_nv12(img, w, h, w, same, 1) == host_encode(img, w, h, w, q, 1)
    for bw, bh in ((33, 18), (34, 17), (0, 18), (65536, 18)):
        with pytest.raises(ValueError):
            jpeg.check_size(bw, bh)
        assert api.jpeg_bound(bw, bh) == 0
    with pytest.raises(ValueError):
        jpeg.check_size(65534, 272, 16)                          # 16 rows of 4096 MCUs
    jpeg.check_size(65534, 272, 15)


def test_inputs_exercise_the_coder():
    """What the GPU tests take from this matrix must be there, or they could pass vacuously."""
    tot = {"stuffed": 0, "zrl": 0, "blocks_without_eob": 0, "edge_blocks_right": 0, "edge_blocks_bottom": 0}
    cats, ac, slices = set(), 0, 0
    for case in matrix():
        st = twin_case(*case)[2]
        for k in tot:
            tot[k] += st[k]
        cats |= st["dc_categories"]
        ac = max(ac, st["max_ac_category"])
        slices = max(slices, st["slices"])
    print(tot, sorted(cats), ac, slices)
    assert tot["stuffed"] >= 50 and tot["zrl"] >= 1 and tot["blocks_without_eob"] >= 1
    assert tot["edge_blocks_right"] >= 1 and tot["edge_blocks_bottom"] >= 1
    assert ac >= 9 and slices > 8
    # DC categories 0 and 11: the latter from 8x8 blocks alternating 0 and 255 at quality 100
    st = twin_case("checker", 96, 64, 96, 100, 1)[2]
    assert {0, 11} <= st["dc_categories"]
    assert twin_case("noise", 48, 160, 48, 95, 1)[2]["slices"] == 10      # RSTm wraps: FF D0 .. FF D7, FF D0
    stream = twin_case("noise", 48, 160, 48, 95, 1)[1]
    assert stream.count(b"\xff\xd0") >= 2


def test_ties_round_to_even():
    """Flat luma blocks of value 128 +- odd at quality 50: the DC quantiser is 16 and its reciprocal 1/128 is exact, so the
    product is exactly on .5.  The stream holds the ties-to-even result, and a ties-away encoder gives other bytes."""
    w, h = 96, 64
    assert jpeg.quant_tables(50)[0][0] == 16 and jpeg.reciprocals(50)[0][0] == np.float32(1.0 / 128.0)
    img = jpeg.sample_image("ties", w, h, w, 5)
    coef = jpeg.dct_coefficients(img, w, h, w)
    luma = np.arange(len(coef)) % 6 < 4
    prod = coef[luma, 0] * jpeg.reciprocals(50)[0][0]
    assert np.all(np.abs(prod - np.floor(prod)) == 0.5)           # every luma DC is a tie
    even = jpeg.encode_nv12(img, w, h, w, 50, 1)
    away = jpeg.encode_nv12(img, w, h, w, 50, 1, rint=jpeg.ties_away)
    assert even == host_encode(img, w, h, w, 50, 1)
    assert even != away
    zz = jpeg.quantise(coef, 50)
    assert np.all(zz[luma, 0] % 2 == 0)


def test_dct_coefficients_layout():
    """coefficient (v, u) at u * 8 + v, AAN-scaled: a horizontal cosine lands in column-frequency u, i.e. at u * 8"""
    w = h = 16
    img = jpeg.sample_image("hf", w, h, w, 0)
    c = jpeg.dct_coefficients(img, w, h, w)
    assert c.shape == (6, 64) and c.dtype == np.float32
    top = np.abs(c[0])                                            # luma block 0: 128 + 100 cos((2x+1) 7 pi / 16), no y term
    assert int(top.argmax()) == 7 * 8 + 0


def test_jpeg_binding_agrees_with_the_header():
    assert int(re.search(r"#define\s+SN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == api.ABI_VERSION == 4      # purely additive
    body = re.search(r"typedef struct sn_jpeg_params \{(.*?)\} sn_jpeg_params;", HEADER, re.S).group(1)
    fields = [(d.split()[1], C.c_int) for d in body.split(";") if d.strip()]
    assert all(d.split()[0] == "int" for d in body.split(";") if d.strip())
    assert fields == list(api.SnJpegParams._fields_) and C.sizeof(api.SnJpegParams) == 8
    lib = api.load_library()
    protos = {
        "sn_jpeg_bound": ("size_t", ["int w", "int h_px"], C.c_size_t),
        "sn_jpeg_encode_nv12": ("int", ["sn_handle *h", "int n", "const uint8_t *nv12", "int w", "int h_px", "int pitch", "size_t frame",
                                        "const sn_jpeg_params *p", "uint8_t *out", "size_t out_stride", "uint32_t *sizes", "int mem",
                                        "void *stream"], C.c_int),
        "sn_dbg_jpeg_dct": ("int", ["sn_handle *h", "const uint8_t *nv12", "int w", "int h_px", "int pitch", "float *out"], C.c_int)}
    special = {"const sn_jpeg_params *p": C.POINTER(api.SnJpegParams), "size_t frame": C.c_size_t, "size_t out_stride": C.c_size_t}
    for name, (ret, params, restype) in protos.items():
        proto = re.search(r"\b%s\s+%s\((.*?)\);" % (ret, name), HEADER, re.S).group(1)
        assert [" ".join(t.split()) for t in proto.split(",")] == params, name
        fn = getattr(lib, name)
        assert fn.restype is restype and len(fn.argtypes) == len(params), name
        for at, prm in zip(fn.argtypes, params):
            assert at is (special[prm] if prm in special else C.c_int if prm.startswith("int ") else C.c_void_p), (name, prm)
    # the header carries the contract: the pass, the quantiser, the markers
    for line in ("z2 = 0.541196100f * o0 + z5;  z4 = 1.306562965f * o2 + z5;  z3 = o1 * 0.707106781f",
                 "recip = (float)(1.0 / (q * aan[u] * aan[v] * 8.0))", "FF D0+(k mod 8) follows slice k, FF D9 the"):
        assert line in HEADER, line
    assert callable(api.StereoNetHIP.jpeg_encode_nv12) and callable(api.StereoNetHIP.jpeg_encode_nv12_device)
    # sn_jpeg_bound needs no device: header + 416 bytes per block + the markers
    assert api.jpeg_bound(1280, 720) >= jpeg.HEADER_BYTES + 6 + 21600 * 416 + 2 * 45
    assert api.jpeg_bound(2, 2) >= jpeg.HEADER_BYTES + 6 * 416 + 2
