"""GPU: adaptive sampling (rtu_render_frame_adaptive) against the CPU oracle's independent statement of the rule
(rtu_oracle_render_adaptive), at the benchmarked shapes and at the edges of the rule.

tests/test_gpu_adaptive.py replays the rule in numpy on images the device made itself; here every pixel, count and counter is
compared with the oracle. The bars:
- counts: the device's count equals the oracle's except where the oracle's margin (the smallest distance between the largest
  channel variance and the target over the checkpoints it evaluated up to its stop: relative for a target > 0, absolute for 0)
  is below 1e-3 (1e-7 absolute), and at 0.1 % of the pixels at most. A decision that close to the target may go either way
  through the last bit of a sample; whichever count the two sides chose, that checkpoint lies among those the oracle evaluated.
- images: the device image against the oracle's mean of each pixel's first n samples at the DEVICE's count n (counts_in), with
  the bars of the fixed renders: test_gpu_sampled.check for recipe S, test_paths_vs_oracle's for recipe P.
- counters: with a target that leaves no pixel borderline, the counting variant equals the oracle's counters with trace_batch =
  the device's batch: a stopped pixel spawns nothing after the batch it stopped in."""
import numpy as np
import pytest

from conftest import PATH_TAGS, SAMPLED_TAGS
from test_gpu_adaptive import mixed_target, same_bits
from test_gpu_fuzz import _make_stochastic, _scene_xml, assets  # noqa: F401 (assets: the fixture of the random scenes)
from test_gpu_parity import check_against
from test_gpu_sampled import check
from test_gpu_workloads import GLASSROOM

pytestmark = pytest.mark.gpu

OT = 16  # oracle threads
RGB8_TOL = 1
BIG = np.float32(1.0e30)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def frame(pkg, scene, W, H, spp, gi, rank=0, count=1, stats=False):
    return pkg.frame_setup(scene.desc.camera, W, H, shard_rank=rank, shard_count=count, samples=spp, gather_bounces=4 if gi else 0,
                           collect_stats=stats)


def render(pkg, ctx, scene, W, H, spp, gi, ad, shards=1):
    """The adaptive frame over `shards` shards, assembled: (rgbz [H, W, 4], counts [H, W])."""
    ctx.upload(scene)
    bufs, frames = [], []
    counts = np.empty((H, W), np.uint8)
    for r in range(shards):
        fr = frame(pkg, scene, W, H, spp, gi, r, shards)
        buf, c, _ = ctx.render_adaptive(fr, ad)
        bufs.append(buf)
        frames.append(fr)
        counts[pkg.shard_global_rows(fr)] = c
    return pkg.assemble(bufs, frames, H), counts


def library_batch(W, H, spp):
    """render_sampled's batch for one shard of W x H pixels: as many samples as fit 2^25 pixels, at most RTU_MAX_BATCH."""
    return max(1, min(16, (1 << 25) // (W * H), spp))


def check_paths(gpu, cpu, orc, what):
    """test_paths_vs_oracle's bars: z bit-exact, z-image equal, 8-bit RGB within +-1, linear RGB to 1e-3 of the value."""
    assert same_bits(gpu[..., 3], cpu[..., 3]), what + ": z differs"
    g8, _, gz8 = orc.postprocess(gpu)
    c8, _, cz8 = orc.postprocess(cpu)
    assert np.array_equal(gz8, cz8), what + ": z-image differs"
    d8 = np.abs(g8.astype(np.int32) - c8.astype(np.int32))
    assert d8.max() <= RGB8_TOL, "%s: 8-bit RGB differs by %d levels at %d pixels" % (what, d8.max(), (d8 > RGB8_TOL).sum())
    d = np.abs(gpu[..., :3].astype(np.float64) - cpu[..., :3].astype(np.float64))
    rel = (d / np.maximum(np.abs(cpu[..., :3]), 1e-2)).max()
    assert rel < 1e-3, "%s: linear RGB differs by %.3g of the value" % (what, rel)


def borderline(margin, target):
    return margin < (np.float32(1e-3) if target > 0 else np.float32(1e-7))


def compare(pkg, orc, scene, W, H, spp, gi, ad, got, counts, what, image_check=None, row0=0, nrows=None):
    """Counts and image of a device frame against the oracle (the bars of the module docstring); returns (oracle counts, margin)."""
    nrows = H - row0 if nrows is None else nrows
    rows = slice(row0, row0 + nrows)
    tv = float(ad.target_variance)
    cpu, ocounts, margin, _ = orc.render_adaptive(scene, W, H, spp, ad.min_samples, ad.increment, tv, gi=gi, counts_in=counts[rows],
                                                  threads=OT, row0=row0, nrows=nrows)
    border = borderline(margin, tv)
    differ = counts[rows] != ocounts
    print("%s: %d pixels, %d borderline, %d differ in count, mean count %.2f" % (what, differ.size, int(border.sum()), int(differ.sum()),
                                                                                 float(counts[rows].mean())))
    bad = differ & ~border
    assert not bad.any(), "%s: %d pixels stop elsewhere than the oracle, clear of the target (first at %s: device %d, oracle %d)" % (
        what, int(bad.sum()), np.argwhere(bad)[0], counts[rows][bad][0], ocounts[bad][0])
    assert differ.sum() <= 1e-3 * differ.size, "%s: %d borderline pixels stop elsewhere" % (what, int(differ.sum()))
    if image_check is not None:
        image_check(got[rows], cpu)
    elif gi:
        check_paths(got[rows], cpu, orc, what)
    else:
        check(got[rows], cpu, orc, spp, what)
    return ocounts, margin


def median_target(orc, scene, W, H, spp, gi, n=4):
    """The median of the non-zero per-pixel variances of the oracle's first n samples: a mixed count map."""
    return mixed_target(orc.sample_images(scene, W, H, spp, 0, n, gi=gi, threads=OT), n)


def clear_target(orc, scene, W, H, spp, gi, mn, inc):
    """A target that leaves no pixel borderline and the count map mixed: of the geometric middles of the widest gaps between the
    largest-channel variances at the checkpoints (the oracle's samples), the one whose smallest relative distance to a variance the
    rule evaluates is largest, among those that stop between 10 % and 90 % of the pixels whose samples disagree at min_samples."""
    imgs = orc.sample_images(scene, W, H, spp, 0, spp, gi=gi, threads=OT)
    s = np.zeros(imgs.shape[1:3] + (3,), np.float32)
    q = np.zeros_like(s)
    vals = []
    for i in range(spp):
        x = imgs[i, ..., :3]
        s = s + x
        q = q + x * x
        n = i + 1
        if 1 < n < spp and n >= mn and (n - mn) % inc == 0:
            vals.append(((q - s * (s / np.float32(n))) / np.float32(n - 1)).max(axis=-1).ravel().astype(np.float64))
    v = np.stack(vals)  # [checkpoint, pixel]
    u = np.unique(v[(v > 0) & np.isfinite(v)])
    u = u[(u >= np.quantile(u, 0.05)) & (u <= np.quantile(u, 0.95))]
    gaps = np.argsort(u[1:] / u[:-1])[::-1][:200]
    varying = v[0] > 0
    best, best_margin = None, 0.0
    for k in gaps:
        t = float(np.float32(np.sqrt(u[k] * u[k + 1])))
        passes = v <= t
        stop = np.where(passes.any(axis=0), passes.argmax(axis=0), len(vals))
        if not 0.1 <= (stop[varying] == 0).mean() <= 0.9:
            continue
        evaluated = np.arange(len(vals))[:, None] <= stop[None, :]
        margin = np.where(evaluated, np.abs(v - t) / t, np.inf).min()
        if margin > best_margin:
            best, best_margin = t, margin
    assert best is not None and best_margin > 2e-3, "no target clear of every pixel's variances (%s, %.3g)" % (best, best_margin)
    return best


def ragged(W, H):
    W, H = W - 3, H - 3
    assert W % 8 and H % 8
    return W, H


# ---- 1. the per-sample images the replay tests rest on ---------------------------------------------------
@pytest.mark.parametrize("tag", ["p10_s4_160x120", "p11_p2_120x68"])
def test_sample_images_match_the_oracle(pkg, orc, ctx, golden, tag):
    """Samples 5 .. 11 of a 32-sample frame at a ragged size over 3 shards: every sample's z bit for bit, RGB within the recipe's bar."""
    g = golden(tag)
    scene = g.scene(pkg)
    gi = tag in PATH_TAGS
    W, H = ragged(g.width, g.height)
    spp, first, n = 32, 5, 7
    ctx.upload(scene)
    frames = [frame(pkg, scene, W, H, spp, gi, r, 3) for r in range(3)]
    shards = [ctx.sample_images(f, first, n) for f in frames]
    cpu = orc.sample_images(scene, W, H, spp, first, n, gi=gi, threads=OT)
    for k in range(n):
        got = pkg.assemble([s[k] for s in shards], frames, H)
        what = "%s %dx%d sample %d" % (tag, W, H, first + k)
        if gi:
            check_paths(got, cpu[k], orc, what)
        else:
            check(got, cpu[k], orc, 1, what)


# ---- 2. every golden stochastic scene ---------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["defaults", "median4"])
@pytest.mark.parametrize("tag", SAMPLED_TAGS + PATH_TAGS)
def test_golden_scene(pkg, orc, ctx, golden, tag, rule):
    """At the golden's size and at a ragged one (width and height not multiples of 8: partial tiles), 32 samples at most, with the
    reference's constants or (4, 2, the median variance at n = 4). The ragged frame over 3 shards is the single frame bit for bit."""
    g = golden(tag)
    scene = g.scene(pkg)
    gi = tag in PATH_TAGS
    spp = 32
    for W, H in ((g.width, g.height), ragged(g.width, g.height)):
        if rule == "defaults":
            ad = pkg.adaptive_defaults()
        else:
            ad = pkg.adaptive_defaults(min_samples=4, increment=2, target_variance=median_target(orc, scene, W, H, spp, gi))
        got, counts = render(pkg, ctx, scene, W, H, spp, gi, ad)
        if rule == "median4":
            assert (counts == 4).any() and (counts > 4).any(), "the count map is not mixed"
        compare(pkg, orc, scene, W, H, spp, gi, ad, got, counts, "%s %dx%d %s" % (tag, W, H, rule))
        if W % 8:
            three, three_counts = render(pkg, ctx, scene, W, H, spp, gi, ad, shards=3)
            assert same_bits(three, got) and np.array_equal(three_counts, counts), "3 shards differ from one"


# ---- 3. the workloads tools/adaptive_bench.py times ---------------------------------------------------------
@pytest.mark.parametrize("tag,size,gi", [("teapot1_s2_160x90", (1920, 1080), False), ("p11_1080", None, True)])
def test_benchmarked_workload(pkg, orc, ctx, golden, tag, size, gi):
    """1920x1080, 64 samples at most, the reference's constants, the library's batch (16 samples, 32 400 tiles in the first
    list, several batches): every pixel and every count against the oracle."""
    g = golden(tag)
    scene = g.scene(pkg)
    W, H = size or (g.width, g.height)
    ad = pkg.adaptive_defaults()
    got, counts = render(pkg, ctx, scene, W, H, 64, gi, ad)
    compare(pkg, orc, scene, W, H, 64, gi, ad, got, counts, "%s %dx%d adaptive 64" % (tag, W, H))


# ---- 4. stopped pixels trace nothing: every counter ---------------------------------------------------------
@pytest.mark.parametrize("B", [1, 4, 0])
@pytest.mark.parametrize("tag", ["teapot1_s2_160x90", "p11_p2_120x68"])
def test_stopped_pixels_trace_nothing_all_counters(pkg, orc, ctx, golden, tag, B):
    """The counting variant with batches of B samples (0: the library's) against the oracle tracing each pixel to the end of the batch
    it stopped in: every counter equal. No pixel is borderline, so every count is the oracle's too."""
    g = golden(tag)
    scene = g.scene(pkg)
    gi = tag in PATH_TAGS
    W, H, spp = g.width, g.height, 20
    t = clear_target(orc, scene, W, H, spp, gi, 4, 2)
    ad = pkg.adaptive_defaults(min_samples=4, increment=2, target_variance=t, max_batch=B)
    cpu, ocounts, margin, ost = orc.render_adaptive(scene, W, H, spp, 4, 2, t, gi=gi, trace_batch=B or library_batch(W, H, spp), threads=OT)
    assert not borderline(margin, t).any(), "%d borderline pixels" % int(borderline(margin, t).sum())
    assert (ocounts == 4).any() and (ocounts > 4).any() and (ocounts % 4 != 0).any()
    ctx.upload(scene)
    fr = frame(pkg, scene, W, H, spp, gi)
    if gi:  # recipe P with counters refuses a capacity overflow: a render without counters settles the capacities
        ctx.render_adaptive(fr, ad)
    got, counts, st = ctx.render_adaptive(fr, ad, stats=True)
    assert np.array_equal(counts, ocounts), "%d pixels stop elsewhere" % int((counts != ocounts).sum())
    if gi:
        check_paths(got, cpu, orc, tag)
    else:
        check(got, cpu, orc, spp, tag)
    assert st == ost, "counters differ: device %s, oracle %s" % (st, ost)


# ---- 5. the edges of the rule -------------------------------------------------------------------------------
EDGES = {  # name: (samples, min_samples, increment, target: a number or the n of a median target)
    "count_255": (255, 254, 1, ("median", 254)),
    "samples_1": (1, 1, 1, 0.005),
    "min_1_finite": (8, 1, 1, ("median", 2)),
    "min_1_inf": (8, 1, 1, float("inf")),
    "one_checkpoint": (16, 5, 12, ("median", 5)),
    "target_0": (16, 4, 2, 0.0),
}


@pytest.mark.parametrize("edge", sorted(EDGES))
def test_edge(pkg, orc, ctx, golden, edge):
    spp, mn, inc, t = EDGES[edge]
    tag = "teapot1_s2_160x90" if edge == "target_0" else "p11gs_s2_160x90"  # (the teapot: pixels that see only the background)
    scene = golden(tag).scene(pkg)
    W, H = 77, 45
    if isinstance(t, tuple):
        t = median_target(orc, scene, W, H, spp, False, t[1])
    ad = pkg.adaptive_defaults(min_samples=mn, increment=inc, target_variance=t)
    got, counts = render(pkg, ctx, scene, W, H, spp, False, ad)
    ocounts, _ = compare(pkg, orc, scene, W, H, spp, False, ad, got, counts, "%s %s" % (tag, edge))
    if edge == "count_255":
        assert (counts == 255).any() and (counts == 254).any()
    elif edge in ("samples_1", "min_1_inf"):
        assert (counts == 1).all() and (ocounts == 1).all()
    elif edge == "min_1_finite":
        assert (counts > 1).all() and (ocounts > 1).all() and (counts == 2).any()
    elif edge == "one_checkpoint":
        assert set(np.unique(counts)) == {5, 16}
    elif edge == "target_0":
        imgs = orc.sample_images(scene, W, H, spp, 0, spp, threads=OT)
        background = (imgs[..., 3] == BIG).all(axis=0)
        assert background.any()
        assert (counts[background] == mn).all() and (ocounts[background] == mn).all()


# ---- 6. a capacity retry inside an adaptive frame -----------------------------------------------------------
def glassroom(pkg, tmp_path):
    """The glass room of test_frame_capacity_overflow_is_detected_and_repaired (up to three child frames per pixel, more frames than
    a fresh context provisions), made stochastic: glossy reflection, a point light with a size."""
    xml = GLASSROOM.replace('<reflection value="0.4"/>', '<reflection value="0.4" glossiness="0.05"/>')
    xml = xml.replace('<light type="point" name="p">', '<light type="point" name="p"><size value="2"/>')
    assert xml.count("glossiness=") == 1 and xml.count("<size") == 1
    path = tmp_path / "glassroom_soft.xml"
    path.write_text(xml)
    return pkg.Scene.from_xml(str(path))


@pytest.mark.parametrize("case", ["s", "s_counters", "p", "after_unread_overflow"])
def test_capacity_retry_in_an_adaptive_frame(pkg, orc, tmp_path, case):
    """On a FRESH context the first batch overflows the frame records. Recipe S without counters renders that batch again (the
    step kernel must have skipped it); with counters the frame starts over (list and sums too); recipe P shades the batch again.
    after_unread_overflow: an asynchronous recipe W frame overflowed and nobody read its status before the adaptive call."""
    scene = glassroom(pkg, tmp_path)
    W, H, spp = 128, 96, 24
    gi = case == "p"
    t = clear_target(orc, scene, W, H, spp, gi, 4, 2)
    ad = pkg.adaptive_defaults(min_samples=4, increment=2, target_variance=t)
    # the asynchronous frame is recipe W: the glass room without its stochastic attributes (overflows a fresh context)
    plain = tmp_path / "glassroom.xml"
    plain.write_text(GLASSROOM)
    hard = pkg.Scene.from_xml(str(plain))
    fw = pkg.frame_setup(hard.desc.camera, W, H)
    if case == "after_unread_overflow":  # the report is there to be missed
        c = pkg.Context(0)
        try:
            c.upload(hard)
            d = pkg.hip.rtu_device_alloc(c._h, W * H * 16)
            c.render_device(fw, d, None)
            with pytest.raises(pkg.RtuError) as e:
                c.frame_status()
            assert e.value.code == pkg.RTU_ERR_CAPACITY
            pkg.hip.rtu_device_free(c._h, d)
        finally:
            c.close()
    c = pkg.Context(0)
    try:
        d = None
        if case == "after_unread_overflow":
            c.upload(hard)
            d = pkg.hip.rtu_device_alloc(c._h, W * H * 16)
            c.render_device(fw, d, None)  # overflows; its status is never read (the upload below leaves the sticky report alone)
        c.upload(scene)
        fr = frame(pkg, scene, W, H, spp, gi, stats=case == "s_counters")
        got, counts, st = c.render_adaptive(fr, ad, stats=case == "s_counters")
        if d is not None:
            pkg.hip.rtu_device_free(c._h, d)
    finally:
        c.close()
    assert (counts == 4).any() and (counts > 4).any()
    ocounts, margin = compare(pkg, orc, scene, W, H, spp, gi, ad, got, counts, "glass room %s" % case)
    assert not borderline(margin, t).any() and np.array_equal(counts, ocounts)
    if case == "s_counters":
        _, _, _, ost = orc.render_adaptive(scene, W, H, spp, 4, 2, t, trace_batch=library_batch(W, H, spp), threads=OT)
        assert st == ost, "counters differ: device %s, oracle %s" % (st, ost)


# ---- 7. random scenes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_random_scene_adaptive(pkg, orc, ctx, assets, seed):  # noqa: F811
    """The stochastic scenes of test_gpu_fuzz.test_random_scene_sampled at 99x61, 16 samples at most, (4, 2, the median variance at
    n = 4; the reference's target where every sample of every pixel agrees).

    Here the device's samples are not always the oracle's bit for bit (deep glass and mirror trees multiply many powf / expf terms;
    measured: samples within 1.04e-3 of the value, a last bit in one channel of one sample), and the median target can be as small as
    2e-8, where one last bit moves a variance by a quarter of the target. So the bars are argued from the samples themselves: the
    device's counts and image are the rule applied exactly to the device's own samples (rtu_debug_sample_images, the same launch
    path), a count may differ from the oracle's only where the two sides' samples differ, at 0.1 % of the pixels at most, and each
    pixel's mean differs from the oracle's by no more than its samples do (plus the rounding of the sums). z is bit-exact and 8-bit
    RGB within +-1 as everywhere."""
    import random
    from test_gpu_adaptive import replay
    rnd = random.Random(7000 + seed)
    textured = seed % 3 == 2
    xml = assets / ("ssa%d.xml" % seed)
    xml.write_text(_make_stochastic(_scene_xml(rnd, assets, textured), rnd))
    scene = pkg.Scene.from_xml(str(xml))
    W, H, spp = 99, 61, 16
    cs = orc.sample_images(scene, W, H, spp, 0, spp, threads=OT)
    try:
        t = mixed_target(cs[:4], 4)
    except AssertionError:  # no pixel whose samples disagree
        t = 0.005
    ad = pkg.adaptive_defaults(min_samples=4, increment=2, target_variance=t)
    got, counts = render(pkg, ctx, scene, W, H, spp, False, ad)
    ds = ctx.sample_images(frame(pkg, scene, W, H, spp, False), 0, spp)
    want, want_counts = replay(ds, 4, 2, t)
    assert np.array_equal(counts, want_counts) and same_bits(got, want), "the device does not apply the rule to its own samples"
    cpu, ocounts, margin, _ = orc.render_adaptive(scene, W, H, spp, 4, 2, t, counts_in=counts, threads=OT)
    assert np.array_equal(replay(cs, 4, 2, t)[1], ocounts)
    n = np.maximum(counts, ocounts).astype(np.int64)
    used = np.arange(spp)[:, None, None] < n[None]
    same_samples = ~((ds.view(np.uint32) != cs.view(np.uint32)).any(-1) & used).any(0)
    differ = counts != ocounts
    print("random scene %d: target %.3g, %d pixels, %d borderline, %d whose samples differ, %d differ in count, mean count %.2f" % (
        seed, t, differ.size, int(borderline(margin, t).sum()), int((~same_samples).sum()), int(differ.sum()), float(counts.mean())))
    assert not (differ & same_samples & ~borderline(margin, t)).any(), "pixels with the oracle's samples stop elsewhere"
    assert differ.sum() <= 1e-3 * differ.size
    check_against(got, cpu, orc, rel_tol=np.inf)  # z, z-image, 8-bit RGB
    k = counts.astype(np.int64)[None, ..., None]
    within = np.arange(spp)[:, None, None, None] < k
    dsum = np.where(within, np.abs(ds[..., :3].astype(np.float64) - cs[..., :3]), 0).sum(0) / k[0]
    asum = np.where(within, np.abs(cs[..., :3].astype(np.float64)), 0).sum(0) / k[0]
    err = np.abs(got[..., :3].astype(np.float64) - cpu[..., :3])
    bound = dsum + 2 * k[0] * 2.0 ** -24 * asum  # the samples' own differences + two sums of k rounded additions
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), "a mean differs from the oracle's by more than its samples do: %.3g > %.3g at %s" % (err[worst], bound[worst], worst)
