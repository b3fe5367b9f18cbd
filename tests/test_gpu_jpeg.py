"""sn_jpeg_encode_nv12 on the MI355X: the transform's fp32 coefficients equal the numpy twin's (hobot_stereonet_amd/jpeg.py) bit
for bit; the streams equal the twin's byte for byte, with equal sizes, over sizes, qualities, restart intervals, pitches and
the contents tests/test_jpeg.py shows to exercise the coder; every call form gives the same bytes; guard words around the
outputs stay untouched; a full-size batch equals the host C++ encoder; a stream that does not fit gives size 0 and writes
nothing; the call runs beside inference; argument errors; the node publishes the same messages with either encoder.

No tolerance appears: the contract is the same bytes."""
import ctypes as C
import functools
import json
import os
import subprocess
import threading

import numpy as np
import pytest

from hobot_stereonet_amd import api, jpeg, synth, weights

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
W, H, D = 96, 64, 48            # the engine's model: the encoder takes its own w and h
MAX_BATCH = 10                  # above the encoder's batch slice of 8 frames, so the walk is exercised
GUARD = 16                      # four guard words
ERR_ARG = -1                    # SN_ERR_ARG (include/stereonet_hip.h)

SIZES = ((96, 64), (70, 50), (34, 18), (132, 70), (48, 160), (2, 2))
QUALITIES = (1, 50, 75, 95, 100)
ROWS = (0, 1, 3, 99)
KINDS = ("noise", "bands", "hf", "checker", "stripes")


def _matrix():
    """every fifth case of tests/test_jpeg.py's product (size x quality x rows x pitch, the content cycling), and the three frames
    the issue names: the ties, DC category 11, white noise at quality 100"""
    i = 0
    for w, h in SIZES:
        for q in QUALITIES:
            for r in ROWS:
                for p in (w, 2 * w, w + 6):
                    if i % 5 == 0:
                        yield KINDS[(i // 5) % len(KINDS)], w, h, p, q, r
                    i += 1
    yield "ties", 96, 64, 96, 50, 1
    yield "checker", 96, 64, 96, 100, 1
    yield "noise", 132, 70, 138, 100, 1
    yield "noise", 48, 160, 48, 95, 1      # ten slices: RSTm wraps


@functools.lru_cache(maxsize=None)
def _twin(kind, w, h, pitch, quality, rows, seed=0):
    img = jpeg.sample_image(kind, w, h, pitch, seed + w + quality)
    img.setflags(write=False)
    return img, jpeg.encode_nv12(img, w, h, pitch, quality, rows)


@pytest.fixture(scope="module")
def eng(model_factory):
    with api.StereoNetHIP(model_factory(W, H, D), max_batch=MAX_BATCH) as e:
        yield e


@functools.lru_cache(maxsize=None)
def _hostlib():
    from hobot_stereonet_amd import build
    build.build()
    subprocess.check_call(["make", "-C", COMPAT, "-s"])
    lib = C.CDLL(os.path.join(COMPAT, "build", "libhobot_stereonet_node.so"))
    lib.snhost_jpeg_nv12_sliced.restype = C.c_long
    lib.snhost_jpeg_nv12_sliced.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long]
    return lib


def _host_encode(img, w, h, pitch, quality, rows) -> bytes:
    src = np.ascontiguousarray(img, np.uint8).reshape(-1)
    buf = np.empty(api.jpeg_bound(w, h), np.uint8)
    n = _hostlib().snhost_jpeg_nv12_sliced(src.ctypes.data, w, h, pitch, quality, rows, buf.ctypes.data, buf.size)
    assert n > 0
    return buf[:n].tobytes()


def _device_call(torch, eng, frames, w, h, pitch, quality, rows, out_stride=0, stream=0, offset=0):
    """device mode on n frames (uint8 (n, rows, pitch)) that start `offset` bytes into their buffer, with four guard words before
    and after `out` and `sizes` -> (list of streams or None, sizes)"""
    n = len(frames)
    flat = np.ascontiguousarray(frames).reshape(-1)
    frame = flat.size // n
    d_in = torch.zeros(flat.size + offset + 4, dtype=torch.uint8, device="cuda")
    d_in[offset:offset + flat.size].copy_(torch.from_numpy(flat.copy()))
    out_stride = out_stride or api.jpeg_bound(w, h)
    d_out = torch.full((n * out_stride + 2 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda")
    d_sz = torch.full((n * 4 + 2 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.jpeg_encode_nv12_device(n, d_in.data_ptr() + offset, w, h, pitch, frame, quality, rows, d_out.data_ptr() + GUARD,
                                out_stride, d_sz.data_ptr() + GUARD, stream=stream)
    if stream:
        torch.cuda.synchronize()
    o, z = d_out.cpu().numpy(), d_sz.cpu().numpy()
    assert np.all(o[:GUARD] == 0x5a) and np.all(o[GUARD + n * out_stride:] == 0x5a), "guard words around out"
    assert np.all(z[:GUARD] == 0x5a) and np.all(z[GUARD + n * 4:] == 0x5a), "guard words around sizes"
    sizes = z[GUARD:GUARD + n * 4].view(np.uint32)
    body = o[GUARD:GUARD + n * out_stride].reshape(n, out_stride)
    streams = [body[k, :sizes[k]].tobytes() if sizes[k] else None for k in range(n)]
    for k in range(n):                                          # nothing behind the stream, nothing at all where it did not fit
        assert np.all(body[k, sizes[k]:] == 0x5a), k
    return streams, sizes


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(70, 50), (96, 64)])
def test_dct_coefficients_equal_twin_bit_for_bit(eng, w, h):
    for kind in ("noise", "bands"):
        for pitch in (w, w + 6):
            img = jpeg.sample_image(kind, w, h, pitch, 7)
            got = eng.dbg_jpeg_dct(img, w, h, pitch)
            want = jpeg.dct_coefficients(img, w, h, pitch)
            differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
            print(f"{kind} {w}x{h} pitch {pitch}: {differ} of {want.size} coefficients differ in a bit")
            assert got.shape == want.shape and differ == 0


@pytest.mark.gpu
def test_streams_equal_twin_byte_for_byte(eng):
    import torch
    bad = []
    cases = list(_matrix())
    for i, (kind, w, h, p, q, r) in enumerate(cases):
        img, want = _twin(kind, w, h, p, q, r)
        got = eng.jpeg_encode_nv12(img, w, h, p, quality=q, rows_per_slice=r)[0]
        if got != want:
            bad.append(("host", kind, w, h, p, q, r, None if got is None else len(got), len(want)))
        if i % 4 == 0:
            dev, sizes = _device_call(torch, eng, img[None], w, h, p, q, r)
            if dev[0] != want or int(sizes[0]) != len(want):
                bad.append(("device", kind, w, h, p, q, r, int(sizes[0]), len(want)))
    print(f"{len(cases)} cases, {len(bad)} differ")
    assert not bad, bad


@pytest.mark.gpu
def test_every_call_form_gives_the_same_bytes(eng):
    import torch
    w, h, q, r = 70, 50, 95, 1
    # side-by-side frames of different content: the left eye at pitch 2w, noise in the right half
    kinds = [("noise", "bands")[k & 1] for k in range(MAX_BATCH)]      # contents that depend on the seed
    frames = np.stack([jpeg.sample_image(kinds[k], w, h, 2 * w, 30 + k) for k in range(MAX_BATCH)])
    want = [jpeg.encode_nv12(frames[k], w, h, 2 * w, q, r) for k in range(MAX_BATCH)]
    assert len(set(want)) == MAX_BATCH
    side = torch.cuda.Stream()
    for n in (1, 3, MAX_BATCH):
        host = eng.jpeg_encode_nv12(frames[:n], w, h, 2 * w, n=n, quality=q, rows_per_slice=r)
        assert host == want[:n], n
        for stream in (0, side.cuda_stream):
            for offset in (0, 1):                                # an odd address
                dev, sizes = _device_call(torch, eng, frames[:n], w, h, 2 * w, q, r, stream=stream, offset=offset)
                assert dev == want[:n] and [int(s) for s in sizes] == [len(s) for s in want[:n]], (n, stream, offset)
    # the same frames, contiguous eyes at pitch w
    eyes = np.ascontiguousarray(frames[:3, :, :w])
    assert eng.jpeg_encode_nv12(eyes, w, h, w, n=3, quality=q, rows_per_slice=r) == want[:3]
    # a raw host buffer and its sizes
    out, sizes = eng.jpeg_encode_nv12(frames[:2], w, h, 2 * w, n=2, quality=q, rows_per_slice=r, raw=True)
    assert out.shape == (2, api.jpeg_bound(w, h)) and [out[k, :sizes[k]].tobytes() for k in range(2)] == want[:2]


@pytest.mark.gpu
def test_full_size_batch_equals_host_encoder(eng):
    import torch
    w, h, n = 1280, 720, 2
    frames = np.stack([synth.sbs_nv12_frame(w, h, 192, 21 + k).reshape(h + h // 2, 2 * w) for k in range(n)])
    for rows in (6, 1):
        want = [_host_encode(frames[k], w, h, 2 * w, 95, rows) for k in range(n)]
        dev, sizes = _device_call(torch, eng, frames, w, h, 2 * w, 95, rows)
        print(f"1280x720 rows_per_slice {rows}: {[int(s) for s in sizes]} bytes")
        assert dev == want and [int(s) for s in sizes] == [len(s) for s in want]
    assert eng.jpeg_encode_nv12(frames, w, h, 2 * w, n=n, quality=95, rows_per_slice=6) == [
        _host_encode(frames[k], w, h, 2 * w, 95, 6) for k in range(n)]


@pytest.mark.gpu
def test_overflow_gives_size_zero_and_writes_nothing(eng):
    import torch
    w, h, q, r = 70, 50, 100, 1
    frames = np.stack([jpeg.sample_image(k, w, h, w, 3) for k in ("bands", "noise", "hf")])
    want = [jpeg.encode_nv12(f, w, h, w, q, r) for f in frames]
    longest = max(range(3), key=lambda k: len(want[k]))
    assert longest == 1
    # one byte short of the noise frame's stream: that frame alone overflows
    stride = len(want[1]) - 1
    assert all(len(want[k]) <= stride for k in (0, 2))
    dev, sizes = _device_call(torch, eng, frames, w, h, w, q, r, out_stride=stride)      # asserts the guards and untouched tails
    assert [int(s) for s in sizes] == [len(want[0]), 0, len(want[2])]
    assert dev == [want[0], None, want[2]]
    host = eng.jpeg_encode_nv12(frames, w, h, w, n=3, quality=q, rows_per_slice=r, out_stride=stride)
    assert host == [want[0], None, want[2]]
    # exactly enough fits
    dev, sizes = _device_call(torch, eng, frames, w, h, w, q, r, out_stride=len(want[1]))
    assert dev == want
    # sn_jpeg_bound holds the worst content
    assert len(want[1]) <= api.jpeg_bound(w, h)
    dev, _ = _device_call(torch, eng, frames[1:2], w, h, w, q, r, out_stride=api.jpeg_bound(w, h))
    assert dev == want[1:2]


@pytest.mark.gpu
def test_encode_beside_submit_and_wait(model_factory):
    """sn_submit tickets in flight while another thread encodes (ctypes drops the GIL): the streams and the maps equal the serial
    run's."""
    xs = [synth.model_input_i8(W, H, D, s) for s in range(4)]
    frames = np.stack([jpeg.sample_image("bands", W, H, 2 * W, 50 + k) for k in range(3)])
    want = [jpeg.encode_nv12(f, W, H, 2 * W, 95, 1) for f in frames]
    with api.StereoNetHIP(model_factory(W, H, D), task_num=4, max_batch=3) as e:
        serial = [e.infer(x)[1] for x in xs]
        errors, rounds = [], []

        def encode():
            try:
                for _ in range(12):
                    if e.jpeg_encode_nv12(frames, W, H, 2 * W, n=3, quality=95, rows_per_slice=1) != want:
                        errors.append("stream differs")
                    rounds.append(1)
            except Exception as ex:        # noqa: BLE001
                errors.append(repr(ex))

        t = threading.Thread(target=encode)
        t.start()
        try:
            for _ in range(5):
                outs = [np.empty((H, W), np.int32) for _ in xs]
                tickets = [e.submit(x, o, None) for x, o in zip(xs, outs)]
                for tk in tickets:
                    e.wait(tk)
                for o, s in zip(outs, serial):
                    assert np.array_equal(o.reshape(s.shape), s)
        finally:
            t.join(60)
        assert not t.is_alive() and not errors and len(rounds) == 12, errors


@pytest.mark.gpu
def test_argument_errors_write_nothing(eng):
    import torch
    lib, hnd = eng._lib, eng._h
    w, h = 34, 18
    img = jpeg.sample_image("bands", w, h, w, 1)
    d_in = torch.from_numpy(img.reshape(-1).copy()).cuda()
    cap = api.jpeg_bound(w, h)
    d_out = torch.full((MAX_BATCH * cap,), 0x5a, dtype=torch.uint8, device="cuda")
    d_sz = torch.full((64,), 0x5a, dtype=torch.uint8, device="cuda")
    prm = api.SnJpegParams(95, 1)

    def call(n=1, src=None, cw=w, ch=h, pitch=w, frame=0, p=prm, out=None, stride=cap, sizes=None, mem=api.SN_MEM_DEVICE):
        src = d_in.data_ptr() if src is None else src
        out = d_out.data_ptr() if out is None else out
        sizes = d_sz.data_ptr() if sizes is None else sizes
        return lib.sn_jpeg_encode_nv12(hnd, n, src or None, cw, ch, pitch, frame, C.byref(p) if p is not None else None, out or None,
                                       stride, sizes or None, mem, None)

    assert call() == 0                                           # the baseline call is fine
    d_out.fill_(0x5a)
    d_sz.fill_(0x5a)
    torch.cuda.synchronize()
    span = (h + h // 2 - 1) * w + w
    bad = {"odd w": dict(cw=33), "odd h": dict(ch=17), "w = 0": dict(cw=0), "h too large": dict(ch=65536), "pitch < w": dict(pitch=w - 2),
           "null input": dict(src=0), "null output": dict(out=0), "null sizes": dict(sizes=0), "null params": dict(p=None),
           "n = 0": dict(n=0), "n > max_batch": dict(n=MAX_BATCH + 1), "bad mem": dict(mem=7),
           "input overlaps out": dict(out=d_in.data_ptr() + span - 1), "input overlaps sizes": dict(sizes=d_in.data_ptr() + 8),
           "out overlaps sizes": dict(sizes=d_out.data_ptr() + 4),
           # 16 rows of 4096 MCUs in a restart interval (the pointer is never followed)
           "restart_mcus > 65535": dict(cw=65534, ch=272, pitch=65534, p=api.SnJpegParams(95, 16))}
    for name, kw in bad.items():
        rc = call(**kw)
        msg = lib.sn_last_error(hnd).decode()
        assert rc == ERR_ARG and "sn_jpeg_encode_nv12" in msg, (name, rc, msg)
    torch.cuda.synchronize()
    assert bool((d_out == 0x5a).all()) and bool((d_sz == 0x5a).all())
    assert call(cw=65534, ch=272, pitch=65534, p=api.SnJpegParams(95, 16), src=0) == ERR_ARG
    assert api.jpeg_bound(33, 18) == 0 and api.jpeg_bound(34, 18) == cap


def _run_node(tmp_path, tag, model, sbs, w, h, nframes, env_extra):
    env = dict(os.environ, SN_LOG_LEVEL="2", **env_extra)      # warnings too: the node names its encoder in one
    prefix = str(tmp_path / tag)
    r = subprocess.run([os.path.join(COMPAT, "build", "node_harness"), model, sbs, str(w), str(h), str(nframes), prefix],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return [open(f"{prefix}.{i}.msg", "rb").read() for i in range(nframes)], r.stderr


@pytest.mark.gpu
def test_node_publishes_identical_messages_with_either_encoder(weights_blob, tmp_path):
    _hostlib()
    w, h, d, nframes = 96, 64, 48, 6
    m = str(tmp_path / "m.snw")
    weights.save_snw(m, weights_blob, w, h, d)
    frame = synth.sbs_nv12_frame(w, h, d, 4)
    frame.tofile(str(tmp_path / "s.bin"))
    for slices in (None, "1"):
        extra = {} if slices is None else {"STEREONET_JPEG_SLICES": slices}
        host, hlog = _run_node(tmp_path, f"host{slices}", m, str(tmp_path / "s.bin"), w, h, nframes, extra)
        gpu, log = _run_node(tmp_path, f"gpu{slices}", m, str(tmp_path / "s.bin"), w, h, nframes, dict(extra, STEREONET_JPEG="gpu"))
        assert "encoder: gpu" in log and "encoder: host" in hlog
        assert all(len(x) > 4 * w * h + 623 for x in host)
        assert gpu == host, slices
        # the picture behind the int32 map is the encoder's stream of the left eye
        rows = 1 if slices is None else 0        # 4 MCU rows in 8 slices -> one row each; one slice -> a single scan
        left = jpeg.encode_nv12(frame.reshape(h + h // 2, 2 * w), w, h, 2 * w, 95, rows)
        assert host[0][4 * w * h:] == left


@pytest.mark.gpu
def test_node_rate_with_the_gpu_encoder_is_recorded(weights_blob, tmp_path):
    """1280x720 through node_harness --bench with four encoder threads, the GPU encoder beside the host encoder: frames/s and the
    process's CPU time per frame, printed, and written into $STEREONET_BENCH_RECORD_DIR when that names a directory.  A measurement;
    the floor only catches a return to the 25 frames/s of an encoder on the
    executor thread (tests/test_host_mirror.py::test_node_level_throughput_is_recorded)."""
    _hostlib()
    w, h, d = 1280, 720, 192
    m = str(tmp_path / "m.snw")
    weights.save_snw(m, weights_blob, w, h, d)
    synth.sbs_nv12_frame(w, h, d, 21).tofile(str(tmp_path / "s.bin"))
    res = {}
    for enc in ("gpu", "host"):
        env = dict(os.environ, SN_LOG_LEVEL="3", STEREONET_JPEG=enc, STEREONET_JPEG_THREADS="4")
        r = subprocess.run([os.path.join(COMPAT, "build", "node_harness"), "--bench", m, str(tmp_path / "s.bin"), str(w), str(h), "400"],
                           capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        print(line)
        res[enc] = json.loads(line)
        out_dir = os.environ.get("STEREONET_BENCH_RECORD_DIR", "")      # where a measuring run keeps its records
        if os.path.isdir(out_dir):
            with open(os.path.join(out_dir, f"node_bench_jpeg_{enc}.json"), "w") as f:
                f.write(line + "\n")
        assert res[enc]["frames"] == 400 and res[enc]["jpeg"] == enc and res[enc]["publish"] is True
        assert res[enc]["frames_per_s"] > 100.0
        assert res[enc]["payload_bytes_per_frame"] > 4 * w * h + 1000
    assert res["gpu"]["payload_bytes_per_frame"] == res["host"]["payload_bytes_per_frame"]


@pytest.mark.gpu
def test_filelist_writes_the_left_eye_jpeg(model_factory, tmp_path, capsys):
    from PIL import Image
    from hobot_stereonet_amd import filelist, images
    rng = np.random.default_rng(11)
    lists = {}
    for eye in ("left", "right"):
        paths = []
        for i in range(2):
            p = str(tmp_path / f"{eye}{i}.ppm")
            images.write_ppm(p, rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
            paths.append(p)
        lists[eye] = str(tmp_path / f"{eye}.list")
        with open(lists[eye], "w") as f:
            f.write("\n".join(paths) + "\n")
    out = str(tmp_path / "out")
    assert filelist.main(["--model", model_factory(W, H, D), "--left", lists["left"], "--right", lists["right"], "--out", out,
                          "--jpeg", "90,2"]) == 0
    total = 0
    for i in range(2):
        eyes = [images.bgr_to_nv12(images.imread_bgr(str(tmp_path / f"{eye}{i}.ppm"))) for eye in ("left", "right")]
        sbs = images.sbs_from_eyes(eyes[0], eyes[1], W, H)
        got = open(os.path.join(out, f"{i}.left.jpg"), "rb").read()
        assert got == jpeg.encode_nv12(sbs, W, H, 2 * W, 90, 2)
        assert Image.open(os.path.join(out, f"{i}.left.jpg")).size == (W, H)
        total += len(got)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["jpeg_bytes"] == total
