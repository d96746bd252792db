"""GPU: adaptive sampling of recipes S and P (rtu_render_frame_adaptive) — a pixel stops at the first checkpoint
n = min_samples + k * increment < samples where (q - s * m) / (n - 1) <= target for r, g and b.

Sample i of a pixel is sample i of the fixed render (same key, same pixel offset) and the sums are formed in sample
order, so everything is checked bit for bit against a numpy replay of the rule on the per-sample images the
accumulator sees (rtu_debug_sample_images). The target of each test is the median of the non-zero per-pixel
variances at n = min_samples, so that the count map is always mixed."""
import ctypes

import numpy as np
import pytest

from conftest import PATH_TAGS, SAMPLED_TAGS

pytestmark = pytest.mark.gpu

BIG = np.float32(1.0e30)
RGB8_TOL = 1


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def frame(pkg, scene, W, H, spp, gather=0, shard_rank=0, shard_count=1, stats=False):
    return pkg.frame_setup(scene.desc.camera, W, H, shard_rank=shard_rank, shard_count=shard_count, collect_stats=stats, samples=spp,
                           gather_bounces=gather)


def mean_of(imgs, n=None):
    """The fixed render's resolve restated: sums in sample order in binary32, rgb = s / n, z = mean z of the hits."""
    n = imgs.shape[0] if n is None else n
    s = np.zeros(imgs.shape[1:3] + (3,), np.float32)
    zs = np.zeros(imgs.shape[1:3], np.float32)
    h = np.zeros(imgs.shape[1:3], np.int64)
    for i in range(n):
        s = s + imgs[i, ..., :3]
        hit = imgs[i, ..., 3] != BIG
        zs = np.where(hit, zs + imgs[i, ..., 3], zs)
        h += hit
    rgb = s / np.float32(n)
    z = np.where(h > 0, zs / np.maximum(h, 1).astype(np.float32), BIG)
    return np.concatenate([rgb, z[..., None]], axis=-1).astype(np.float32)


def variance_at(imgs, n):
    s = np.zeros(imgs.shape[1:3] + (3,), np.float32)
    q = np.zeros_like(s)
    for i in range(n):
        x = imgs[i, ..., :3]
        s = s + x
        q = q + x * x
    if n == 1:
        return np.full(s.shape, np.inf, np.float32)
    m = s / np.float32(n)
    return (q - s * m) / np.float32(n - 1)


def replay(imgs, min_samples, increment, target):
    """The stopping rule of rtu_render.h on the per-sample images: (rgbz, counts)."""
    S = imgs.shape[0]
    shape = imgs.shape[1:3]
    s = np.zeros(shape + (3,), np.float32)
    q = np.zeros_like(s)
    zs = np.zeros(shape, np.float32)
    h = np.zeros(shape, np.int64)
    counts = np.full(shape, S, np.int64)
    live = np.ones(shape, bool)
    target = np.float32(target)
    for i in range(S):
        x = imgs[i, ..., :3]
        s = np.where(live[..., None], s + x, s)
        q = np.where(live[..., None], q + x * x, q)
        hit = live & (imgs[i, ..., 3] != BIG)
        zs = np.where(hit, zs + imgs[i, ..., 3], zs)
        h += hit
        n = i + 1
        if n < S and n >= min_samples and (n - min_samples) % increment == 0:
            if n == 1:
                var = np.full(s.shape, np.inf, np.float32)
            else:
                var = (q - s * (s / np.float32(n))) / np.float32(n - 1)
            stop = live & np.all(var <= target, axis=-1)
            counts[stop] = n
            live &= ~stop
    rgb = s / counts.astype(np.float32)[..., None]
    z = np.where(h > 0, zs / np.maximum(h, 1).astype(np.float32), BIG)
    return np.concatenate([rgb, z[..., None]], axis=-1).astype(np.float32), counts.astype(np.uint8)


def mixed_target(imgs, min_samples):
    v = variance_at(imgs, min_samples).max(axis=-1)
    nz = v[(v > 0) & np.isfinite(v)]
    assert nz.size > 0, "the scene has no pixel whose samples disagree"
    return float(np.median(nz))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def setup(pkg, ctx, golden, tag, spp, gather, min_samples=4, increment=2):
    g = golden(tag)
    scene = g.scene(pkg)
    ctx.upload(scene)
    fr = frame(pkg, scene, g.width, g.height, spp, gather)
    imgs = ctx.sample_images(fr, 0, spp)
    target = mixed_target(imgs, min_samples)
    ad = pkg.adaptive_defaults(min_samples=min_samples, increment=increment, target_variance=target)
    return g, scene, fr, imgs, ad


def check_replay(pkg, ctx, fr, imgs, ad):
    fixed, _ = ctx.render(fr)
    assert same_bits(mean_of(imgs), fixed), "the per-sample images do not average to the fixed render"
    got, counts, _ = ctx.render_adaptive(fr, ad)
    want, want_counts = replay(imgs, ad.min_samples, ad.increment, ad.target_variance)
    assert (counts == ad.min_samples).any() and (counts > ad.min_samples).any(), "the count map is not mixed"
    assert np.array_equal(counts, want_counts), "%d pixels stop elsewhere" % int((counts != want_counts).sum())
    assert same_bits(got, want), "%d pixels differ from the replay" % int((got.view(np.uint32) != want.view(np.uint32)).any(-1).sum())
    return got, counts


def check_limits(pkg, ctx, fr, ad):
    fixed, _ = ctx.render(fr)
    full = pkg.adaptive_defaults(min_samples=fr.samples, increment=ad.increment, target_variance=0.0)
    got, counts, _ = ctx.render_adaptive(fr, full)
    assert (counts == fr.samples).all()
    assert same_bits(got, fixed)
    inf = pkg.adaptive_defaults(min_samples=ad.min_samples, increment=ad.increment, target_variance=float("inf"))
    got, counts, _ = ctx.render_adaptive(fr, inf)
    assert (counts == ad.min_samples).all()


def check_counting(pkg, ctx, fr, ad, B):
    """With batches of B samples a pixel that stops at n was traced ceil(n / B) * B times (at most `samples`): the counting variant
    counts exactly those primary rays — a stopped pixel spawns nothing — and renders the fast variant's image."""
    adb = pkg.adaptive_defaults(min_samples=ad.min_samples, increment=ad.increment, target_variance=ad.target_variance, max_batch=B)
    fast, fast_counts, _ = ctx.render_adaptive(fr, adb)
    got, counts, st = ctx.render_adaptive(fr, adb, stats=True)
    assert np.array_equal(counts, fast_counts)
    assert same_bits(got, fast)
    n = counts.astype(np.int64)
    traced = np.minimum(fr.samples, B * ((n + B - 1) // B))
    assert st["primary_rays"] == int(traced.sum()), (st["primary_rays"], int(traced.sum()), fr.samples * n.size)
    assert st["primary_rays"] < fr.samples * n.size


# ---- recipe S --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["p10_s4_160x120", "teapot1_s2_160x90"])
def test_replay_recipe_s(pkg, ctx, golden, tag):
    assert tag in SAMPLED_TAGS
    _, _, fr, imgs, ad = setup(pkg, ctx, golden, tag, 32, 0)
    check_replay(pkg, ctx, fr, imgs, ad)


def test_limits_recipe_s(pkg, ctx, golden):
    _, _, fr, _, ad = setup(pkg, ctx, golden, "p9_s3_160x120", 32, 0)
    check_limits(pkg, ctx, fr, ad)


def test_batch_size_changes_nothing(pkg, ctx, golden):
    _, _, fr, _, ad = setup(pkg, ctx, golden, "p11gs_s2_160x90", 40, 0, min_samples=5, increment=3)
    ref, ref_counts, _ = ctx.render_adaptive(fr, ad)
    assert (ref_counts == 5).any() and (ref_counts > 5).any()
    for B in (1, 3, 0, pkg.RTU_MAX_BATCH):
        adb = pkg.adaptive_defaults(min_samples=5, increment=3, target_variance=ad.target_variance, max_batch=B)
        got, counts, _ = ctx.render_adaptive(fr, adb)
        assert np.array_equal(counts, ref_counts), "max_batch %d" % B
        assert same_bits(got, ref), "max_batch %d" % B


def test_shards_assemble_to_one(pkg, ctx, golden):
    g, scene, fr, _, ad = setup(pkg, ctx, golden, "p10_s4_160x120", 32, 0)
    one, one_counts, _ = ctx.render_adaptive(fr, ad)
    shards, frames, cshards = [], [], []
    for r in range(3):
        f = frame(pkg, scene, g.width, g.height, 32, 0, shard_rank=r, shard_count=3)
        buf, counts, _ = ctx.render_adaptive(f, ad)
        assert buf.shape[0] == pkg.hip.rtu_shard_rows(ctypes.byref(f)) == counts.shape[0]
        shards.append(buf)
        frames.append(f)
        cshards.append(counts)
    assert same_bits(pkg.assemble(shards, frames, g.height), one)
    counts = np.empty_like(one_counts)
    for c, f in zip(cshards, frames):
        counts[pkg.shard_global_rows(f)] = c
    assert np.array_equal(counts, one_counts)


def test_stopped_pixels_trace_nothing(pkg, ctx, golden):
    _, _, fr, _, ad = setup(pkg, ctx, golden, "teapot1_s2_160x90", 32, 0)
    check_counting(pkg, ctx, fr, ad, 4)


def test_device_entry(pkg, ctx, golden):
    _, _, fr, _, ad = setup(pkg, ctx, golden, "p11x86_s1_120x90", 32, 0)
    want, want_counts, _ = ctx.render_adaptive(fr, ad)
    rows = pkg.hip.rtu_shard_rows(ctypes.byref(fr))
    n = rows * fr.width
    d = pkg.hip.rtu_device_alloc(ctx._h, n * 16)
    dc = pkg.hip.rtu_device_alloc(ctx._h, n)
    try:
        ctx._check(pkg.hip.rtu_render_frame_adaptive_device(ctx._h, ctypes.byref(fr), ctypes.byref(ad), d, dc, None))
        assert pkg.hip.rtu_frame_status(ctx._h) == pkg.RTU_OK
        got = np.empty((rows, fr.width, 4), np.float32)
        counts = np.empty((rows, fr.width), np.uint8)
        ctx._check(pkg.hip.rtu_copy_to_host(ctx._h, got.ctypes.data, d, n * 16))
        ctx._check(pkg.hip.rtu_copy_to_host(ctx._h, counts.ctypes.data, dc, n))
    finally:
        pkg.hip.rtu_device_free(ctx._h, d)
        pkg.hip.rtu_device_free(ctx._h, dc)
    assert same_bits(got, want)
    assert np.array_equal(counts, want_counts)


def test_pixels_at_the_maximum_match_the_oracle(pkg, orc, ctx, golden):
    """A pixel that went to `samples` is the fixed render's pixel: against the oracle at spp = samples with test_gpu_sampled's bars."""
    from test_gpu_sampled import check
    g, scene, fr, _, ad = setup(pkg, ctx, golden, "p10_s4_160x120", 32, 0)
    got, counts, _ = ctx.render_adaptive(fr, ad)
    cpu, _ = orc.render_samples(scene, g.width, g.height, 32, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=8)
    at_max = counts == 32
    assert at_max.any()
    check(np.where(at_max[..., None], got, cpu), cpu, orc, 32, "adaptive pixels at the maximum")


# ---- recipe P --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def paths_case(pkg, ctx, golden):
    tag = PATH_TAGS[0]
    return setup(pkg, ctx, golden, tag, 32, 4)


def test_replay_recipe_p(pkg, ctx, paths_case):
    g, scene, fr, imgs, ad = paths_case
    ctx.upload(scene)
    check_replay(pkg, ctx, fr, imgs, ad)


def test_limits_recipe_p(pkg, ctx, paths_case):
    g, scene, fr, imgs, ad = paths_case
    ctx.upload(scene)
    check_limits(pkg, ctx, fr, ad)


def test_stopped_chains_trace_nothing(pkg, ctx, paths_case):
    g, scene, fr, imgs, ad = paths_case
    ctx.upload(scene)
    # recipe P with counters refuses a capacity overflow: the capacities are settled by a render without counters first
    adb = pkg.adaptive_defaults(min_samples=ad.min_samples, increment=ad.increment, target_variance=ad.target_variance, max_batch=4)
    ctx.render_adaptive(fr, adb)
    check_counting(pkg, ctx, fr, ad, 4)


def test_paths_pixels_at_the_maximum_match_the_oracle(pkg, orc, ctx, paths_case):
    g, scene, fr, imgs, ad = paths_case
    ctx.upload(scene)
    got, counts, _ = ctx.render_adaptive(fr, ad)
    cpu, _ = orc.render_paths(scene, g.width, g.height, 32, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=8)
    at_max = counts == 32
    assert at_max.any()
    mixed = np.where(at_max[..., None], got, cpu)
    assert same_bits(mixed[..., 3], cpu[..., 3]), "z differs"
    g8, _, gz8 = orc.postprocess(mixed)
    c8, _, cz8 = orc.postprocess(cpu)
    assert np.array_equal(gz8, cz8)
    assert np.abs(g8.astype(np.int32) - c8.astype(np.int32)).max() <= RGB8_TOL


# ---- arguments, cancel, BeginRender ---------------------------------------------------------------------
def test_refusals(pkg, ctx, golden):
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    ctx.upload(scene)
    W, H = g.width, g.height
    ok = pkg.adaptive_defaults(min_samples=2)

    def rc(fr, ad):
        out = np.empty((pkg.hip.rtu_shard_rows(ctypes.byref(fr)), W, 4), np.float32)
        return pkg.hip.rtu_render_frame_adaptive(ctx._h, ctypes.byref(fr), ctypes.byref(ad) if ad is not None else None, out.ctypes.data, None, None)

    fr = frame(pkg, scene, W, H, 4)
    assert rc(fr, ok) == pkg.RTU_OK
    assert rc(fr, None) == pkg.RTU_ERR_ARG
    for spp in (0, 256):  # (0: a recipe W frame is no adaptive frame)
        assert rc(frame(pkg, scene, W, H, spp), pkg.adaptive_defaults(min_samples=1)) == pkg.RTU_ERR_ARG
    for kw in ({"min_samples": 0}, {"min_samples": 5}, {"increment": 0}, {"increment": -2}, {"target_variance": float("nan")},
               {"target_variance": -1e-6}, {"max_batch": -1}, {"max_batch": pkg.RTU_MAX_BATCH + 1}):
        assert rc(fr, pkg.adaptive_defaults(**dict({"min_samples": 2}, **kw))) == pkg.RTU_ERR_ARG, kw
    bad = frame(pkg, scene, W, H, 4)
    bad.gather_bounces = 2
    assert rc(bad, ok) == pkg.RTU_ERR_ARG
    out = np.empty((4, H, W, 4), np.float32)
    assert pkg.hip.rtu_debug_sample_images(ctx._h, ctypes.byref(fr), 1, 4, out.ctypes.data) == pkg.RTU_ERR_ARG  # past frame.samples
    assert pkg.hip.rtu_debug_sample_images(ctx._h, ctypes.byref(frame(pkg, scene, W, H, 0)), 0, 1, out.ctypes.data) == pkg.RTU_ERR_ARG


def test_cancel(pkg, ctx, golden):
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    ctx.upload(scene)
    flag = ctypes.c_int(1)
    pkg.hip.rtu_set_cancel_flag(ctx._h, ctypes.byref(flag))
    try:
        with pytest.raises(pkg.RtuError) as e:
            ctx.render_adaptive(frame(pkg, scene, g.width, g.height, 16), pkg.adaptive_defaults(min_samples=2))
        assert e.value.code == pkg.RTU_ERR_CANCELLED
    finally:
        pkg.hip.rtu_set_cancel_flag(ctx._h, None)
    ctx.render_adaptive(frame(pkg, scene, g.width, g.height, 16), pkg.adaptive_defaults(min_samples=2))  # and renders again


@pytest.mark.parametrize("gather", [0, 4])
def test_begin_render_adaptive(pkg, ctx, golden, gather, tmp_path):
    """main.cpp:59-63 with the sample-count lines: Result.png, ZBuffer.png and SampleCount.png are the post-processed adaptive image
    and its counts, on one device and on three contexts of it (three shards)."""
    from conftest import read_png
    tag = "p10_s4_160x120" if gather == 0 else PATH_TAGS[0]
    spp = 24
    g, scene, fr, imgs, ad = setup(pkg, ctx, golden, tag, spp, gather)
    got, counts, _ = ctx.render_adaptive(fr, ad)
    want = pkg.Image(g.width, g.height)
    want.fill(got)
    want.compute_zimage()
    want.fill_sample_count(counts)
    assert want.compute_sample_count_image() == counts.max()
    outs = []
    for devices in ([0], [0, 0, 0]):
        img = pkg.Image(g.width, g.height)
        d = tmp_path / ("n%d" % len(devices))
        d.mkdir()
        paths = [str(d / n) for n in ("Result.png", "ZBuffer.png", "SampleCount.png")]
        devs = (ctypes.c_int * len(devices))(*devices)
        job = pkg.host.rtu_begin_render_adaptive(scene._h, img._h, devs, len(devices), spp, gather, ctypes.byref(ad), *[p.encode() for p in paths])
        assert job
        assert pkg.host.rtu_render_wait(job) == 0, pkg.host.rtu_host_last_error()
        pkg.host.rtu_render_job_free(job)
        r, z, c = (read_png(p) for p in paths)
        assert np.array_equal(r, want.pixels())
        assert np.array_equal(z, want.zimage())
        assert np.array_equal(c, want.sample_count_image())
        assert np.array_equal(img.sample_count(), counts)
        outs.append((r, z, c))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
