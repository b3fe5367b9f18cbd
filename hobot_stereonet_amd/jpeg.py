"""The numpy twin of the JPEG encoder: the readable statement of the contract that sn_jpeg_encode_nv12 (csrc/sn_jpeg.hpp) and the
host C++ encoder (csrc/compat/src/jpeg_nv12.cpp, EncodeNv12ToJpegSliced: the authority) both meet byte for byte.

Baseline JPEG straight from NV12: YCbCr 4:2:0, 16x16 MCUs (Y0 Y1 Y2 Y3 Cb Cr), the Annex K quantisation tables scaled by the
IJG quality rule, the Annex K Huffman tables, an optional restart interval of `rows_per_slice` MCU rows.

The transform is float32 operation by operation in the order of the host's aan_pass (no fused multiply-add): vertical pass,
transpose, vertical pass again, which leaves coefficient (v, u) at [u][v]; quantisation is one float32 multiply by the
reciprocal (float)(1 / (q * aan[u] * aan[v] * 8)) and np.rint (ties to even).  Entropy coding is in integers."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                   41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
Q_LUM = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
                  14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                  18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHR = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                  99, 99, 47, 66] + [99] * 38)
DC_LUM_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHR_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUM_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUM_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
AC_CHR_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHR_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
AAN = [1.0, 1.387039845, 1.306562965, 1.175875602, 1.0, 0.785694958, 0.541196100, 0.275899379]
HEADER_BYTES = 623      # + 6 with a DRI segment

_F = np.float32
_C707, _C382, _C541, _C1306 = _F(0.707106781), _F(0.382683433), _F(0.541196100), _F(1.306562965)


def _huff(bits, vals):
    """-> (code[256], length[256]); a symbol the table does not hold has length 0"""
    code, length = [0] * 256, [0] * 256
    c = k = 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            code[vals[k]], length[vals[k]] = c, ln
            c += 1
            k += 1
        c <<= 1
    return code, length


HUFF = {"dc_lum": _huff(DC_LUM_BITS, DC_VALS), "dc_chr": _huff(DC_CHR_BITS, DC_VALS),
        "ac_lum": _huff(AC_LUM_BITS, AC_LUM_VALS), "ac_chr": _huff(AC_CHR_BITS, AC_CHR_VALS)}


def clamp_quality(q: int) -> int:
    return 1 if q < 1 else 100 if q > 100 else int(q)


def quant_tables(quality: int):
    """-> (luma, chroma) quantisers in natural order, after the IJG scaling"""
    q = clamp_quality(quality)
    sf = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * sf + 50) // 100, 1, 255).astype(np.int64) for t in (Q_LUM, Q_CHR))


def zigzag_source():
    """zigzag position i -> index into the transposed coefficient block the two passes leave"""
    return (ZIGZAG & 7) * 8 + (ZIGZAG >> 3)


def reciprocals(quality: int):
    """-> (luma, chroma) float32 reciprocal quantisers in zigzag order"""
    out = []
    for q in quant_tables(quality):
        out.append(np.array([1.0 / (float(q[nat]) * (AAN[nat & 7] * AAN[nat >> 3] * 8.0)) for nat in ZIGZAG], np.float32))
    return tuple(out)


def mcu_rows(h: int) -> int:
    return (h + 15) // 16


def restart_mcus(w: int, h: int, rows_per_slice: int) -> int:
    """MCUs per restart interval; 0: a single scan without DRI"""
    return 0 if rows_per_slice <= 0 or rows_per_slice >= mcu_rows(h) else rows_per_slice * ((w + 15) // 16)


def check_size(w: int, h: int, rows_per_slice: int = 0):
    if not (2 <= w <= 65535 and 2 <= h <= 65535) or (w & 1) or (h & 1):
        raise ValueError(f"jpeg: {w}x{h}: width and height must be even and within 2..65535")
    if restart_mcus(w, h, rows_per_slice) > 65535:
        raise ValueError("jpeg: more than 65535 MCUs per restart interval")


def header(w: int, h: int, quality: int, restart: int) -> bytes:
    """SOI, APP0, two DQT, SOF0, four DHT, DRI when restart > 0, SOS"""
    ql, qc = quant_tables(quality)
    o = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t, q in enumerate((ql, qc)):
        o += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(int(q[z]) for z in ZIGZAG)
    o += b"\xff\xc0\x00\x11\x08" + bytes([h >> 8, h & 255, w >> 8, w & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    for cls, bits, vals in ((0x00, DC_LUM_BITS, DC_VALS), (0x10, AC_LUM_BITS, AC_LUM_VALS), (0x01, DC_CHR_BITS, DC_VALS),
                            (0x11, AC_CHR_BITS, AC_CHR_VALS)):
        n = 3 + 16 + len(vals)
        o += b"\xff\xc4" + bytes([n >> 8, n & 255, cls]) + bytes(bits) + bytes(vals)
    if restart > 0:
        o += b"\xff\xdd\x00\x04" + bytes([restart >> 8, restart & 255])
    o += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    return bytes(o)


def _image(nv12, w, h, pitch):
    a = np.ascontiguousarray(nv12, np.uint8).reshape(-1)
    rows = h + h // 2
    need = (rows - 1) * pitch + w
    if pitch < w or a.size < need:
        raise ValueError(f"jpeg: a {w}x{h} NV12 image at pitch {pitch} takes {need} bytes, the buffer has {a.size}")
    return np.lib.stride_tricks.as_strided(a, (rows, w), (pitch, 1), writeable=False)


def blocks(nv12, w: int, h: int, pitch: int) -> np.ndarray:
    """The level-shifted samples of every 8x8 block in coding order -> float32 (mcus * 6, 8, 8).  Blocks cut by the right or
    bottom edge replicate the last column or row; the chroma planes are w/2 x h/2, read interleaved."""
    img = _image(nv12, w, h, pitch)
    mw, mh = (w + 15) // 16, mcu_rows(h)
    ys = np.minimum(np.arange(mh * 16), h - 1)
    xs = np.minimum(np.arange(mw * 16), w - 1)
    luma = img[:h][np.ix_(ys, xs)].reshape(mh, 2, 8, mw, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(mh * mw, 4, 8, 8)
    cy = np.minimum(np.arange(mh * 8), h // 2 - 1)
    cx = np.minimum(np.arange(mw * 8), w // 2 - 1)
    out = np.empty((mh * mw, 6, 8, 8), np.float32)
    out[:, :4] = luma
    for comp in (0, 1):
        plane = img[h:, comp::2][np.ix_(cy, cx)]
        out[:, 4 + comp] = plane.reshape(mh, 8, mw, 8).transpose(0, 2, 1, 3).reshape(mh * mw, 8, 8)
    return (out - _F(128.0)).reshape(-1, 8, 8)


def aan_pass(d: np.ndarray) -> np.ndarray:
    """One AAN 8-point DCT along axis 1 of float32 (N, 8, 8), in the host code's order of operations"""
    r = [d[:, i, :] for i in range(8)]
    t0, t7 = r[0] + r[7], r[0] - r[7]
    t1, t6 = r[1] + r[6], r[1] - r[6]
    t2, t5 = r[2] + r[5], r[2] - r[5]
    t3, t4 = r[3] + r[4], r[3] - r[4]
    e0, e3, e1, e2 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = np.empty_like(d)
    o[:, 0], o[:, 4] = e0 + e1, e0 - e1
    z1 = (e2 + e3) * _C707
    o[:, 2], o[:, 6] = e3 + z1, e3 - z1
    o0, o1, o2 = t4 + t5, t5 + t6, t6 + t7
    z5 = (o0 - o2) * _C382
    z2 = _C541 * o0 + z5
    z4 = _C1306 * o2 + z5
    z3 = o1 * _C707
    z11, z13 = t7 + z3, t7 - z3
    o[:, 5], o[:, 3] = z13 + z2, z13 - z2
    o[:, 1], o[:, 7] = z11 + z4, z11 - z4
    assert o.dtype == np.float32
    return o


def dct_coefficients(nv12, w: int, h: int, pitch: int) -> np.ndarray:
    """The fp32 coefficients before quantisation, float32 (blocks, 64), in the transposed layout the two passes leave them in
    (coefficient (v, u) at u * 8 + v, with the AAN scale factors still in): what sn_dbg_jpeg_dct returns."""
    check_size(w, h)
    a = aan_pass(blocks(nv12, w, h, pitch))
    return aan_pass(np.ascontiguousarray(a.transpose(0, 2, 1))).reshape(-1, 64)


def quantise(coef: np.ndarray, quality: int, rint=np.rint) -> np.ndarray:
    """float32 (blocks, 64) -> int64 (blocks, 64) in zigzag order; blocks 4 and 5 of every six are chroma.  rint: the rounding
    (the contract's is np.rint, ties to even; the tests pass another to show that a case tells them apart)"""
    rl, rc = reciprocals(quality)
    z = coef[:, zigzag_source()]
    recip = np.where((np.arange(len(z)) % 6 >= 4)[:, None], rc[None, :], rl[None, :]).astype(np.float32)
    prod = z * recip
    assert prod.dtype == np.float32
    return rint(prod).astype(np.int64)


def _category(v: int) -> int:
    return int(abs(v)).bit_length()


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code: int, length: int):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length

    def drain(self):
        k = self.n >> 3
        if k:
            self.n -= 8 * k
            self.out += (self.acc >> self.n).to_bytes(k, "big")
            self.acc &= (1 << self.n) - 1

    def finish(self) -> bytes:      # pad the last partial byte with ones
        if self.n & 7:
            pad = 8 - (self.n & 7)
            self.put((1 << pad) - 1, pad)
        self.drain()
        return bytes(self.out)


def _encode_slice(zz: np.ndarray, st: dict) -> bytes:
    """The stuffed entropy-coded bytes of the blocks zz (a whole number of MCUs), DC predictors starting at 0"""
    bw = _Bits()
    pred = [0, 0, 0]
    nzmask = zz != 0
    for b in range(len(zz)):
        j = b % 6
        comp = 0 if j < 4 else j - 3
        dc, ac = (HUFF["dc_lum"], HUFF["ac_lum"]) if comp == 0 else (HUFF["dc_chr"], HUFF["ac_chr"])
        row = zz[b]
        diff = int(row[0]) - pred[comp]
        pred[comp] = int(row[0])
        nb = _category(diff)
        st["dc_categories"].add(nb)
        bw.put(dc[0][nb], dc[1][nb])
        if nb:
            bw.put(diff + (1 << nb) - 1 if diff < 0 else diff, nb)
        prev = 0
        for i in np.flatnonzero(nzmask[b, 1:]) + 1:
            i = int(i)
            run = i - prev - 1
            prev = i
            while run > 15:
                bw.put(ac[0][0xF0], ac[1][0xF0])
                st["zrl"] += 1
                run -= 16
            v = int(row[i])
            nb = _category(v)
            st["max_ac_category"] = max(st["max_ac_category"], nb)
            sym = (run << 4) | nb
            bw.put(ac[0][sym], ac[1][sym])
            bw.put(v + (1 << nb) - 1 if v < 0 else v, nb)
        if prev != 63:
            bw.put(ac[0][0], ac[1][0])
        else:
            st["blocks_without_eob"] += 1
        bw.drain()
    raw = bw.finish()
    st["stuffed"] += raw.count(b"\xff")
    return raw.replace(b"\xff", b"\xff\x00")


def _cut(size: int, mcus: int, per_mcu: int = 2) -> int:
    """of the mcus * per_mcu blocks along one axis of a plane of `size` samples, those that reach beyond its edge"""
    return sum(1 for c in range(mcus * per_mcu) if c * 8 + 8 > size)


def _encode(nv12, w, h, pitch, quality, rows_per_slice, rint=np.rint):
    check_size(w, h, rows_per_slice)
    quality = clamp_quality(quality)
    mw, rows = (w + 15) // 16, mcu_rows(h)
    st = {"stuffed": 0, "zrl": 0, "blocks_without_eob": 0, "dc_categories": set(), "max_ac_category": 0, "slices": 1,
          "bytes": 0, "blocks": mw * rows * 6,
          "edge_blocks_right": _cut(w, mw) * 2 * rows + _cut(w // 2, mw, 1) * 2 * rows,
          "edge_blocks_bottom": _cut(h, rows) * 2 * mw + _cut(h // 2, rows, 1) * 2 * mw}
    zz = quantise(dct_coefficients(nv12, w, h, pitch), quality, rint)
    restart = restart_mcus(w, h, rows_per_slice)
    out = bytearray(header(w, h, quality, restart))
    if not restart:
        out += _encode_slice(zz, st) + b"\xff\xd9"
    else:
        st["slices"] = (rows + rows_per_slice - 1) // rows_per_slice
        for k, r in enumerate(range(0, rows, rows_per_slice)):
            r1 = min(r + rows_per_slice, rows)
            out += _encode_slice(zz[r * mw * 6:r1 * mw * 6], st)
            out += bytes([0xFF, 0xD0 + (k & 7) if r1 < rows else 0xD9])
    st["bytes"] = len(out)
    return bytes(out), st


def encode_nv12(nv12, w: int, h: int, pitch: int, quality: int, rows_per_slice: int, rint=np.rint) -> bytes:
    """The stream of EncodeNv12ToJpegSliced: rows_per_slice <= 0 or >= ceil(h / 16) is a single scan without DRI; otherwise
    header, slice 0, FF D0, slice 1, FF D1, ... (RSTm counts modulo 8), last slice, FF D9."""
    return _encode(nv12, w, h, pitch, quality, rows_per_slice, rint)[0]


def stats(nv12, w: int, h: int, pitch: int, quality: int, rows_per_slice: int) -> dict:
    """What the stream of encode_nv12 exercises: stuffed FF 00 pairs, ZRL symbols, blocks that end on coefficient 63 (no EOB),
    the set of DC categories, the largest AC category, slices, blocks with edge-replicated samples (right, bottom), bytes."""
    return _encode(nv12, w, h, pitch, quality, rows_per_slice)[1]


def ties_away(x: np.ndarray) -> np.ndarray:
    """round half away from zero: NOT the contract's rounding (see quantise)"""
    return np.sign(x) * np.floor(np.abs(x) + np.float32(0.5))


IMAGE_KINDS = ("noise", "bands", "hf", "checker", "stripes", "ties")


def sample_image(kind: str, w: int, h: int, pitch: int, seed: int = 0) -> np.ndarray:
    """The contents the encoder's tests use -> uint8 (h * 3/2, pitch), noise beside the image where pitch > w.
      noise    white noise: the entropy coder's worst case (stuffed 0xFF bytes, blocks without EOB)
      bands    band-limited content with a little noise
      hf       128 + 100 cos((2x+1) 7 pi / 16), in the lower half times the same in y: one coefficient far out in zigzag order
               (ZRL), and coefficient 63 (no EOB)
      checker  8x8 luma blocks alternating 0 and 255 (DC category 11 at quality 100), flat chroma (DC category 0)
      stripes  luma columns alternating 0 and 255 (large AC categories)
      ties     flat 8x8 luma blocks of value 128 +- odd: at quality 50 (DC quantiser 16, reciprocal exactly 1/128) the DC
               product sits exactly on .5"""
    rng = np.random.default_rng(seed)
    rows = h + h // 2
    img = rng.integers(0, 256, (rows, pitch), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return img
    if kind == "bands":
        y = 128 + 60 * np.sin(xx / 9.0 + seed) + 50 * np.cos(yy / 7.0) + rng.integers(-3, 4, (h, w))
        uv = 128 + 40 * np.sin(np.mgrid[0:h // 2, 0:w][1] / 13.0) + rng.integers(-2, 3, (h // 2, w))
    elif kind == "hf":
        cx = np.cos((2 * (xx % 8) + 1) * 7 * np.pi / 16)
        cy = np.where(yy >= h // 2, np.cos((2 * (yy % 8) + 1) * 7 * np.pi / 16), 1.0)
        y = 128 + 100 * cx * cy
        uv = np.full((h // 2, w), 128.0)
    elif kind == "checker":
        y = np.where(((xx >> 3) + (yy >> 3)) & 1, 255.0, 0.0)
        uv = np.full((h // 2, w), 128.0)
    elif kind == "stripes":
        y = np.where(xx & 1, 255.0, 0.0)
        uv = np.where(np.mgrid[0:h // 2, 0:w][1] & 2, 255.0, 0.0)
    elif kind == "ties":
        odd = 2 * rng.integers(-30, 30, ((h + 7) // 8, (w + 7) // 8)) + 1
        y = 128 + odd[yy >> 3, xx >> 3]
        uv = np.full((h // 2, w), 128.0)
    else:
        raise ValueError(kind)
    img[:h, :w] = np.clip(np.rint(y), 0, 255).astype(np.uint8)
    img[h:, :w] = np.clip(np.rint(uv), 0, 255).astype(np.uint8)
    return img
