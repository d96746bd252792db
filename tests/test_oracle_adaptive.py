"""CPU-only: the oracle's adaptive sampling (rtu_oracle_render_adaptive) and per-sample images (rtu_oracle_render_sample_images)
against the oracle's own fixed renders and a numpy replay of the stopping rule of include/rtu_render.h.

The adaptive entry shares every line that traces and shades with render_samples / render_paths; what it adds is the rule, the
returned prefix mean and the tracing past a stop that models the device's batches. These tests pin each of the three, so that
tests/test_gpu_adaptive_oracle.py can compare the device with it."""
import numpy as np
import pytest

from test_gpu_adaptive import mean_of, mixed_target, replay, same_bits

T = 8  # oracle threads


def fixed(orc, scene, W, H, spp, gi, **kw):
    f = orc.render_paths if gi else orc.render_samples
    return f(scene, W, H, spp, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=T, **kw)


def prefix_mean(imgs, counts):
    """Per pixel the fixed resolve of its first counts[p] samples (mean_of restated with a count per pixel)."""
    S = imgs.shape[0]
    s = np.zeros(imgs.shape[1:3] + (3,), np.float32)
    zs = np.zeros(imgs.shape[1:3], np.float32)
    h = np.zeros(imgs.shape[1:3], np.int64)
    for i in range(S):
        take = counts > i
        s = np.where(take[..., None], s + imgs[i, ..., :3], s)
        hit = take & (imgs[i, ..., 3] != np.float32(1.0e30))
        zs = np.where(hit, zs + imgs[i, ..., 3], zs)
        h += hit
    rgb = s / counts.astype(np.float32)[..., None]
    z = np.where(h > 0, zs / np.maximum(h, 1).astype(np.float32), np.float32(1.0e30))
    return np.concatenate([rgb, z[..., None]], axis=-1).astype(np.float32)


CASES = [("p10_s4_160x120", False, None), ("teapot1_s2_160x90", False, None), ("p11_p2_120x68", True, None),
         ("p10_s4_160x120", False, (157, 93))]


@pytest.mark.parametrize("rule", [(4, 2), (8, 1)])
@pytest.mark.parametrize("tag,gi,size", CASES)
def test_adaptive_equals_replay_of_its_sample_images(pkg, orc, golden, tag, gi, size, rule):
    """The rule on the oracle's own sample images, replayed in numpy: rgbz and counts bit for bit. The images themselves average
    to the fixed render bit for bit."""
    g = golden(tag)
    scene = g.scene(pkg)
    W, H = size or (g.width, g.height)
    spp = 24
    mn, inc = rule
    imgs = orc.sample_images(scene, W, H, spp, 0, spp, gi=gi, threads=T)
    assert same_bits(mean_of(imgs), fixed(orc, scene, W, H, spp, gi)[0]), "the sample images do not average to the fixed render"
    target = mixed_target(imgs, mn)
    got, counts, margin, _ = orc.render_adaptive(scene, W, H, spp, mn, inc, target, gi=gi, threads=T)
    want, want_counts = replay(imgs, mn, inc, target)
    assert (counts == mn).any() and (counts > mn).any() and (counts == spp).any(), "the count map is not mixed"
    assert np.array_equal(counts, want_counts), "%d pixels stop elsewhere" % int((counts != want_counts).sum())
    assert same_bits(got, want), "%d pixels differ from the replay" % int((got.view(np.uint32) != want.view(np.uint32)).any(-1).sum())
    assert (margin >= 0).all() and np.isfinite(margin).all()  # every pixel has at least one checkpoint with a finite variance


def test_sample_image_window(pkg, orc, golden):
    """A window [first, first + n) is that slice of the whole stack, in rows [row0, row0 + nrows) too."""
    g = golden("p11_p2_120x68")
    scene = g.scene(pkg)
    W, H, spp = 117, 67, 12
    full = orc.sample_images(scene, W, H, spp, 0, spp, gi=True, threads=T)
    assert same_bits(orc.sample_images(scene, W, H, spp, 5, 7, gi=True, threads=3), full[5:12])
    assert same_bits(orc.sample_images(scene, W, H, spp, 3, 2, gi=True, threads=T, row0=21, nrows=9), full[3:5, 21:30])
    for bad in ((-1, 2), (11, 2), (0, 0)):
        with pytest.raises(orc.OracleError):
            orc.sample_images(scene, W, H, spp, bad[0], bad[1])


@pytest.mark.parametrize("tag,gi", [("p9_s3_160x120", False), ("p13_p2_96x72", True)])
def test_counts_in(pkg, orc, golden, tag, gi):
    """counts_in = spp everywhere is the fixed render bit for bit, counters included (trace_batch 1 traces exactly the samples it
    returns); mixed counts_in return each pixel's prefix mean and leave the rule's counts alone."""
    g = golden(tag)
    scene = g.scene(pkg)
    W, H, spp = g.width, g.height, 16
    want, wst = fixed(orc, scene, W, H, spp, gi)
    target = 1e-3
    _, rule_counts, rule_margin, _ = orc.render_adaptive(scene, W, H, spp, 4, 2, target, gi=gi, threads=T)
    got, counts, margin, st = orc.render_adaptive(scene, W, H, spp, 4, 2, target, gi=gi, threads=T, counts_in=np.full((H, W), spp, np.uint8))
    assert same_bits(got, want)
    assert st == wst
    assert np.array_equal(counts, rule_counts) and same_bits(margin, rule_margin)
    mixed = np.random.default_rng(5).integers(1, spp + 1, size=(H, W)).astype(np.uint8)
    got, counts, margin, _ = orc.render_adaptive(scene, W, H, spp, 4, 2, target, gi=gi, threads=T, counts_in=mixed)
    imgs = orc.sample_images(scene, W, H, spp, 0, spp, gi=gi, threads=T)
    assert same_bits(got, prefix_mean(imgs, mixed))
    assert np.array_equal(counts, rule_counts) and same_bits(margin, rule_margin)
    for bad in (0, spp + 1):
        c = mixed.copy()
        c[3, 4] = bad
        with pytest.raises(orc.OracleError):
            orc.render_adaptive(scene, W, H, spp, 4, 2, target, gi=gi, counts_in=c)


@pytest.mark.parametrize("tag,gi", [("teapot1_s2_160x90", False), ("p11_p2_120x68", True)])
def test_trace_batch_stats(pkg, orc, golden, tag, gi):
    """trace_batch = spp traces every sample: the fixed render's counters. Smaller batches trace less, never more, and exactly
    min(spp, B * ceil(n / B)) primary rays per pixel."""
    g = golden(tag)
    scene = g.scene(pkg)
    W, H, spp = g.width, g.height, 20
    _, wst = fixed(orc, scene, W, H, spp, gi)
    imgs = orc.sample_images(scene, W, H, spp, 0, 4, gi=gi, threads=T)
    target = mixed_target(imgs, 4)
    prev, ref = None, None
    for B in (1, 4, spp):
        got, counts, _, st = orc.render_adaptive(scene, W, H, spp, 4, 2, target, gi=gi, trace_batch=B, threads=T)
        if ref is None:
            ref = (got, counts)
            assert (counts == 4).any() and (counts > 4).any()
        assert same_bits(got, ref[0]) and np.array_equal(counts, ref[1]), "trace_batch %d changes the result" % B
        n = counts.astype(np.int64)
        assert st["primary_rays"] == int(np.minimum(spp, B * ((n + B - 1) // B)).sum()), B
        if prev is not None:
            assert all(st[k] >= prev[k] for k in st), (B, st, prev)
        prev = st
    assert prev == wst


def test_threads_and_rows(pkg, orc, golden):
    """One thread or many, the whole frame or row bands: the same rgbz, counts, margins and (summed) counters."""
    g = golden("p11x86_s1_120x90")
    scene = g.scene(pkg)
    W, H, spp = 117, 87, 16
    args = (scene, W, H, spp, 3, 3, mixed_target(orc.sample_images(scene, W, H, spp, 0, 3, threads=T), 3))
    one = orc.render_adaptive(*args, trace_batch=4, threads=1)
    many = orc.render_adaptive(*args, trace_batch=4, threads=7)
    parts = [orc.render_adaptive(*args, trace_batch=4, threads=3, row0=r0, nrows=nr) for r0, nr in ((0, 40), (40, 1), (41, 46))]
    assert (one[1] == 3).any() and (one[1] > 3).any()
    for other in (many, tuple(np.concatenate([p[i] for p in parts]) for i in range(3)) + ({k: sum(p[3][k] for p in parts) for k in one[3]},)):
        assert same_bits(other[0], one[0])
        assert np.array_equal(other[1], one[1])
        assert same_bits(other[2], one[2])
        assert other[3] == one[3]


def test_edges(pkg, orc, golden):
    """samples 1; min_samples 1 with a finite target (n = 1 has variance +inf: no pixel stops there) and with +inf (all stop at 1);
    a single checkpoint; samples 255 with min_samples 254, so that the count reaches 255."""
    g = golden("p11gs_s2_160x90")
    scene = g.scene(pkg)
    W, H = 61, 37
    imgs = orc.sample_images(scene, W, H, 255, 0, 255, threads=T)
    one, _ = fixed(orc, scene, W, H, 1, False)
    got, counts, margin, _ = orc.render_adaptive(scene, W, H, 1, 1, 1, 0.0, threads=T)
    assert (counts == 1).all() and same_bits(got, one) and np.isinf(margin).all()
    _, counts, _, _ = orc.render_adaptive(scene, W, H, 8, 1, 1, mixed_target(imgs, 2), threads=T)
    assert (counts >= 2).all() and (counts == 2).any()
    got, counts, _, _ = orc.render_adaptive(scene, W, H, 8, 1, 1, float("inf"), threads=T)
    assert (counts == 1).all()
    assert same_bits(got, orc.render_adaptive(scene, W, H, 8, 1, 1, 0.0, threads=T, counts_in=np.ones((H, W), np.uint8))[0])
    _, counts, _, _ = orc.render_adaptive(scene, W, H, 16, 5, 12, mixed_target(imgs, 5), threads=T)
    assert set(np.unique(counts)) == {5, 16}
    target = mixed_target(imgs, 254)
    got, counts, _, _ = orc.render_adaptive(scene, W, H, 255, 254, 1, target, threads=T)
    want, want_counts = replay(imgs, 254, 1, target)
    assert set(np.unique(counts)) == {254, 255}
    assert np.array_equal(counts, want_counts) and same_bits(got, want)


def test_refusals(pkg, orc, golden):
    scene = golden("p10_s4_160x120").scene(pkg)
    for kw in ({"spp": 0}, {"spp": 256}, {"min_samples": 0}, {"min_samples": 9}, {"increment": 0}, {"target": -1.0},
               {"target": float("nan")}, {"trace_batch": 0}):
        a = dict(spp=8, min_samples=2, increment=1, target=0.01, trace_batch=1)
        a.update(kw)
        with pytest.raises(orc.OracleError):
            orc.render_adaptive(scene, 16, 16, a["spp"], a["min_samples"], a["increment"], a["target"], trace_batch=a["trace_batch"])
