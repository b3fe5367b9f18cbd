"""The numpy twin of sn_smooth_raw (hobot_stereonet_amd/smooth.py) against a per-pixel loop written straight from the header
text (tests/golden/plain_refs.py), hand-computed answers, the weight table, and the invariants of mask and counts.  No GPU."""
import numpy as np
import pytest

from hobot_stereonet_amd import smooth
from plain_refs import smooth_brute as brute

IMAX, IMIN = 2 ** 31 - 1, -2 ** 31


def random_map(rng, w=24, h=16):
    """invalid and negative pixels, ties (few distinct values), values up to INT32_MAX; luma with flat regions and edges"""
    vals = np.array([IMIN, -3, 0, 0, 1, 2, 2, 1000, 1001, 1001, 40000, IMAX - 1, IMAX, IMAX], np.int64)
    raw = vals[rng.integers(0, len(vals), (h, w))].astype(np.int32)
    raw[:, w // 2:] = rng.integers(-20000, 60000, (h, w - w // 2))
    luma = rng.integers(0, 256, (h, w)).astype(np.uint8)
    luma[: h // 2] = (luma[: h // 2] // 64) * 3 + 100          # nearly flat: differences of 0..9
    return raw, luma


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("sigma", [0, 1, 12, 255])
def test_twin_equals_the_per_pixel_loop(radius, sigma):
    rng = np.random.default_rng(100 * radius + sigma)
    raw, luma = random_map(rng)
    for min_valid in (0, 1, (2 * radius + 1) ** 2 // 2):
        out, mask, counts = smooth.reference(raw, luma, radius, sigma, min_valid)
        b_out, b_mask = brute(raw, luma, radius, sigma, min_valid)
        assert np.array_equal(out, b_out), (radius, sigma, min_valid)
        assert np.array_equal(mask, b_mask), (radius, sigma, min_valid)
        assert out.dtype == np.int32 and mask.dtype == np.uint8 and counts.dtype == np.uint32 and counts.shape == (1, 3)


def test_weights_change_the_answer_against_the_plain_median():
    # the centre's luma side holds 10, 10, 10, 10 (with the centre), the other side five values of 50
    raw = np.array([[10, 50, 50], [10, 10, 50], [10, 50, 50]], np.int32)
    luma = np.array([[20, 200, 200], [20, 20, 200], [20, 200, 200]], np.uint8)
    plain, _, _ = smooth.reference(raw, None, 1, 0, 0)
    assert plain[1, 1] == 50                                   # sorted 10 x4, 50 x5: the fifth of nine
    guided, gmask, _ = smooth.reference(raw, luma, 1, 12, 0)
    # T[0] = 256, T[180] = 36864 // 32544 = 1: Wt = 4 * 256 + 5 = 1029, the 10s carry 1024 >= 514.5
    assert smooth.weight_table(12)[180] == 1
    assert guided[1, 1] == 10 and gmask[1, 1] == 0


def test_even_count_takes_the_lower_median():
    raw = np.array([[0, 7, 0], [0, 3, 0], [0, 0, 0]], np.int32)
    out, mask, counts = smooth.reference(raw, None, 1, 0, 0)
    assert out[1, 1] == 3 and out[0, 1] == 3                   # {3, 7}: cumulative 1 of 2 reaches half at 3
    assert mask[1, 1] == 0 and mask[0, 1] == 128
    assert counts.tolist() == [[2, 1, 0]]
    raw4 = np.array([[5, 9, 0], [1, 7, 0], [0, 0, 0]], np.int32)
    assert smooth.reference(raw4, None, 1, 0, 0)[0][1, 1] == 5   # {1, 5, 7, 9}: the second of four


def test_window_is_clipped_at_a_corner():
    raw = np.array([[9, 1, 100], [2, 8, 100], [100, 100, 100]], np.int32)
    out, _, _ = smooth.reference(raw, None, 1, 0, 0)
    assert out[0, 0] == 2                                      # {9, 1, 2, 8} only: sorted 1 2 8 9, the second; no padding values
    out3, _, _ = smooth.reference(np.full((2, 2), 6, np.int32), None, 3, 0, 0)
    assert np.all(out3 == 6)                                   # a window larger than the image


def test_invalid_centre_below_and_at_min_valid():
    raw = np.array([[4, 0, 0], [0, -1, 0], [6, 0, 5]], np.int32)
    for mv, want, bits in ((4, 0, 1), (3, 5, 129), (0, 0, 1)):
        out, mask, counts = smooth.reference(raw, None, 1, 0, mv)
        assert out[1, 1] == want and mask[1, 1] == bits, mv
    out, mask, counts = smooth.reference(raw, None, 1, 0, 3)
    assert counts[0, 2] == int(((mask & 128 != 0) & (raw <= 0)).sum()) >= 1


def test_invalid_centre_whose_luma_is_far_from_every_neighbour_stays_zero():
    raw = np.full((3, 3), 500, np.int32)
    raw[1, 1] = 0
    luma = np.full((3, 3), 10, np.uint8)
    luma[1, 1] = 250
    assert smooth.weight_table(1)[240] == 0
    out, mask, counts = smooth.reference(raw, luma, 1, 1, 1)
    assert out[1, 1] == 0 and mask[1, 1] == 1                  # 8 measured neighbours >= min_valid, but Wt = 0
    assert np.array_equal(out, raw) and counts.tolist() == [[8, 0, 0]]
    luma[1, 1] = 12                                            # T[2] = 256 // 5 = 51 > 0: now it is filled
    out, mask, _ = smooth.reference(raw, luma, 1, 1, 1)
    assert out[1, 1] == 500 and mask[1, 1] == 129


def test_weight_table():
    t1 = smooth.weight_table(1)
    assert t1[:5].tolist() == [256, 128, 51, 25, 15] and t1[15] == 1 and t1[16] == 0 and not t1[16:].any()
    t255 = smooth.weight_table(255)
    assert t255[0] == 256 and t255[1] == 255 and t255[255] == 128 and t255[128] == (256 * 65025) // (65025 + 16384) == 204
    assert np.all(np.diff(t255) <= 0) and np.all(np.diff(t1) <= 0)
    assert smooth.weight_table(0).tolist() == [1] * 256
    assert t1.dtype == np.int32 and t1.shape == (256,)
    with pytest.raises(ValueError):
        smooth.weight_table(256)


def test_mask_values_and_counts():
    rng = np.random.default_rng(5)
    raw, luma, _ = smooth.noisy_scene(96, 64, 1)
    maps = np.stack([raw, random_map(rng, 96, 64)[0]])
    lum = np.stack([luma, random_map(rng, 96, 64)[1]])
    out, mask, counts = smooth.reference(maps, lum, 2, 12, 5)
    assert set(np.unique(mask).tolist()) == {0, 1, 128, 129}
    assert np.array_equal(out > 0, np.isin(mask, (0, 128, 129)))
    assert np.array_equal(mask & 1 != 0, maps <= 0)
    assert np.array_equal(mask & 128 != 0, out != np.maximum(maps, 0))
    for k in range(2):
        assert counts[k].tolist() == [int((out[k] > 0).sum()), int((mask[k] == 128).sum()), int((mask[k] == 129).sum())]
    one = smooth.reference(maps[1], lum[1], 2, 12, 5)              # a batch is its maps, each on its own
    assert np.array_equal(one[0], out[1]) and np.array_equal(one[1], mask[1]) and np.array_equal(one[2][0], counts[1])


def test_constant_map_is_a_fixed_point():
    raw = np.full((20, 33), 12345, np.int32)
    luma = np.random.default_rng(2).integers(0, 256, raw.shape).astype(np.uint8)
    for radius, sigma in ((1, 0), (2, 12), (3, 1)):
        out, mask, counts = smooth.reference(raw, luma, radius, sigma, 3)
        assert np.array_equal(out, raw) and not mask.any() and counts.tolist() == [[raw.size, 0, 0]]


def test_twice_the_same_bytes():
    raw, luma, _ = smooth.noisy_scene(96, 64, 3)
    a = smooth.reference(raw, luma, 2, 12, 5)
    b = smooth.reference(raw.copy(), luma.copy(), 2, 12, 5)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_luma_helpers_and_expected_disp():
    rng = np.random.default_rng(8)
    w, h = 10, 5                                                   # an odd height: ceil(h / 2) chroma rows
    y = rng.integers(0, 256, (2, h, w)).astype(np.uint8)
    ten = rng.integers(-128, 128, (2, 6, h, w)).astype(np.int8)
    ten[:, 0] = (y ^ 0x80).view(np.int8)
    assert np.array_equal(smooth.luma_from_tensor(ten), y) and np.array_equal(smooth.luma_from_tensor(ten[1]), y[1])
    for pitch in (w, 2 * w):
        frame = pitch * (h + 3)
        buf = rng.integers(0, 256, 2 * frame).astype(np.uint8)
        for k in range(2):
            for v in range(h):
                buf[k * frame + v * pitch:k * frame + v * pitch + w] = y[k, v]
        assert np.array_equal(smooth.luma_from_nv12(buf, w, h, pitch, 2), y)
    assert np.array_equal(smooth.luma_from_nv12(y[0], w, h), y[:1])    # the luma rows alone are enough for one frame
    disp0 = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint32).view(np.float32)
    out = np.arange(h * w, dtype=np.int32).reshape(h, w)
    mask = np.where(out % 2 == 0, 128, 1).astype(np.uint8)
    d = smooth.expected_disp(disp0, out, mask).view(np.uint32)
    assert np.array_equal(d[mask == 1], disp0.view(np.uint32)[mask == 1])
    assert d[0, 0] == 0 and np.array_equal(d[mask == 128].view(np.float32)[1:],
                                           (out[mask == 128].astype(np.float32) * smooth.wire_scale())[1:])
