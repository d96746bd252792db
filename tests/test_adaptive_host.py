"""CPU: the host side of adaptive sampling — the sample-count image of the RenderImage mirror
(RenderImage::ComputeSampleCountImage / SaveSampleCountImage, scene.h:614-640) and the reference's
sampling constants (RenderFunctions.cpp:26-29)."""
import numpy as np
import pytest


def sample_count_image_ref(counts):
    """scene.h:614-635 restated: smin / smax over the uchar counts, 255 * (c - smin) / (smax - smin) in integers,
    clamped; all zero when smax == smin. Returns (image, smax)."""
    c = counts.astype(np.int64)
    smin, smax = int(c.min()), int(c.max())
    if smax == smin:
        return np.zeros(counts.shape, np.uint8), smax
    return np.clip((255 * (c - smin)) // (smax - smin), 0, 255).astype(np.uint8), smax


def test_defaults_are_the_reference_constants(pkg):
    d = pkg.adaptive_defaults()
    assert (d.min_samples, d.increment, d.max_batch) == (8, 1, 0)
    assert d.target_variance == np.float32(0.005)
    assert pkg.hip.rtu_adaptive_defaults(None) == pkg.RTU_ERR_ARG


def test_sample_counts_start_at_zero(pkg):
    img = pkg.Image(13, 7)
    assert img.sample_count_image() is None  # nothing computed yet
    assert not img.sample_count().any()
    assert img.compute_sample_count_image() == 0
    assert not img.sample_count_image().any()


@pytest.mark.parametrize("seed,lo,hi", [(1, 0, 256), (2, 8, 65), (3, 200, 256), (4, 17, 19)])
def test_sample_count_image_matches_reference(pkg, seed, lo, hi):
    rng = np.random.default_rng(seed)
    W, H = 37, 23
    counts = rng.integers(lo, hi, size=(H, W)).astype(np.uint8)
    img = pkg.Image(W, H)
    # filled band by band, as the shards arrive
    for r0 in range(0, H, 8):
        img.fill_sample_count(counts[r0:r0 + 8], r0)
    assert np.array_equal(img.sample_count(), counts)
    want, smax = sample_count_image_ref(counts)
    assert img.compute_sample_count_image() == smax
    assert np.array_equal(img.sample_count_image(), want)


@pytest.mark.parametrize("value", [0, 8, 64, 255])
def test_sample_count_image_all_equal(pkg, value):
    img = pkg.Image(9, 5)
    img.fill_sample_count(np.full((5, 9), value, np.uint8), 0)
    assert img.compute_sample_count_image() == value
    assert not img.sample_count_image().any()  # smax == smin: all zero


def test_sample_count_png_round_trip(pkg, tmp_path):
    from conftest import read_png
    rng = np.random.default_rng(7)
    W, H = 41, 19
    counts = rng.integers(8, 65, size=(H, W)).astype(np.uint8)
    img = pkg.Image(W, H)
    path = str(tmp_path / "SampleCount.png")
    with pytest.raises(pkg.RtuError):
        img.save_sample_count(path)  # SaveSampleCountImage needs the computed image
    img.fill_sample_count(counts, 0)
    img.compute_sample_count_image()
    img.save_sample_count(path)
    got = read_png(path)
    assert got.dtype == np.uint8 and got.shape == (H, W)  # 8-bit grey
    assert np.array_equal(got, img.sample_count_image())
    assert np.array_equal(got, sample_count_image_ref(counts)[0])


def test_begin_render_adaptive_refuses_bad_arguments(pkg):
    import ctypes
    img = pkg.Image(8, 8)
    devs = (ctypes.c_int * 1)(0)
    assert not pkg.host.rtu_begin_render_adaptive(None, img._h, devs, 1, 16, 0, None, None, None, None)
