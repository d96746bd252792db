"""GPU: progressive rendering (rtu_progressive_*, rtu_begin_render_progressive): a recipe S / P frame refined call by call.

After every pass a snapshot is the mean of each pixel's first n samples (n = samples done; adaptive: the pixel's own count) — checked
bit for bit against the device's own per-sample images reduced in numpy in sample order (k_accumulate's sums, k_resolve's divisions),
and against the CPU oracle at those counts with the bars of the fixed renders. A session driven to the end is the one-shot image bit for
bit, whatever the schedule; other renders on the same context between passes change nothing on either side."""
import ctypes
import gc
import threading

import numpy as np
import pytest

from conftest import PATH_TAGS, read_png
from test_gpu_adaptive import mixed_target
from test_gpu_sampled import check

pytestmark = pytest.mark.gpu

OT = 16  # oracle threads
BIG = np.float32(1.0e30)
RGB8_TOL = 1


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def frame(pkg, scene, W, H, spp, gi, rank=0, count=1):
    return pkg.frame_setup(scene.desc.camera, W, H, shard_rank=rank, shard_count=count, samples=spp, gather_bounces=4 if gi else 0)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def prefix_mean(imgs, n):
    """k_accumulate's sums of samples [0, n) in sample order, then k_resolve's divisions, in binary32."""
    s = np.zeros(imgs.shape[1:3] + (3,), np.float32)
    zs = np.zeros(imgs.shape[1:3], np.float32)
    hits = np.zeros(imgs.shape[1:3], np.uint32)
    for k in range(n):
        s = s + imgs[k, ..., :3]
        hit = imgs[k, ..., 3] != BIG
        zs = np.where(hit, zs + imgs[k, ..., 3], zs)
        hits = hits + hit
    out = np.empty(imgs.shape[1:3] + (4,), np.float32)
    out[..., :3] = s / np.float32(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[..., 3] = np.where(hits > 0, zs / hits.astype(np.float32), BIG)
    return out


def prefix_mean_counts(imgs, counts):
    """k_adaptive_step's sums: samples [0, counts[p]) of every pixel in sample order, then k_resolve_counts's divisions."""
    s = np.zeros(imgs.shape[1:3] + (3,), np.float32)
    zs = np.zeros(imgs.shape[1:3], np.float32)
    hits = np.zeros(imgs.shape[1:3], np.uint32)
    for k in range(int(counts.max())):
        on = k < counts
        s = np.where(on[..., None], s + imgs[k, ..., :3], s)
        hit = on & (imgs[k, ..., 3] != BIG)
        zs = np.where(hit, zs + imgs[k, ..., 3], zs)
        hits = hits + hit
    out = np.empty(imgs.shape[1:3] + (4,), np.float32)
    out[..., :3] = s / counts.astype(np.float32)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        out[..., 3] = np.where(hits > 0, zs / hits.astype(np.float32), BIG)
    return out


def check_paths(gpu, cpu, orc, what):
    """The recipe-P bars of test_paths_vs_oracle: z bit-exact, z-image equal, 8-bit RGB within +-1, linear RGB to 1e-3 of the value."""
    assert same_bits(gpu[..., 3], cpu[..., 3]), what + ": z differs"
    g8, _, gz8 = orc.postprocess(gpu)
    c8, _, cz8 = orc.postprocess(cpu)
    assert np.array_equal(gz8, cz8), what + ": z-image differs"
    d8 = np.abs(g8.astype(np.int32) - c8.astype(np.int32))
    assert d8.max() <= RGB8_TOL, "%s: 8-bit RGB differs by %d levels" % (what, d8.max())
    d = np.abs(gpu[..., :3].astype(np.float64) - cpu[..., :3].astype(np.float64))
    assert (d / np.maximum(np.abs(cpu[..., :3]), 1e-2)).max() < 1e-3, what + ": linear RGB differs"


def drive(sess, schedule):
    snaps = []
    for n in schedule:
        sess.advance(n)
        snaps.append(sess.snapshot())
    return snaps


# ---- 1. exact prefix means ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["p10_s4_160x120", "teapot1_s2_160x90", "p11_p2_120x68"])
def test_snapshots_are_prefix_means(pkg, orc, ctx, golden, tag):
    """Passes of 1, 2, 3 and 7 samples of a 16-sample frame: each snapshot is, bit for bit, the numpy mean of the device's own sample
    images [0, done), and it meets the oracle's image at counts = done (recipe S bars / recipe P bars). p10 is textured."""
    g = golden(tag)
    scene = g.scene(pkg)
    gi = tag in PATH_TAGS
    W, H, S = g.width, g.height, 16
    ctx.upload(scene)
    fr = frame(pkg, scene, W, H, S, gi)
    imgs = ctx.sample_images(fr, 0, 13)
    sess = ctx.progressive(fr)
    done = 0
    for n in (1, 2, 3, 7):
        sess.advance(n)
        done += n
        assert sess.status() == (done, (W + 7) // 8 * ((H + 7) // 8))
        got, counts = sess.snapshot()
        assert (counts == done).all()
        assert same_bits(got, prefix_mean(imgs, done)), "%s: snapshot after %d samples is not the mean of samples [0, %d)" % (tag, done, done)
        cpu, _, _, _ = orc.render_adaptive(scene, W, H, S, 1, 1, 0.0, gi=gi, counts_in=np.full((H, W), done, np.uint8), threads=OT)
        what = "%s after %d samples" % (tag, done)
        if gi:
            check_paths(got, cpu, orc, what)
        else:
            check(got, cpu, orc, done, what)
    sess.close()


# ---- 2. the end of a session is the one-shot frame ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["p10_s4_160x120", "p11_p2_120x68"])
def test_fixed_session_ends_at_the_one_shot_image(pkg, ctx, golden, tag):
    g = golden(tag)
    scene = g.scene(pkg)
    gi = tag in PATH_TAGS
    S = 12
    ctx.upload(scene)
    fr = frame(pkg, scene, g.width, g.height, S, gi)
    want, _ = ctx.render(fr)
    for schedule in ([S], [1, 1, 2, 4, 4], [1] * S):
        sess = ctx.progressive(fr)
        got, counts = drive(sess, schedule)[-1]
        assert sess.status() == (S, 0)
        assert same_bits(got, want), "%s: schedule %s does not end at the one-shot image" % (tag, schedule)
        assert (counts == S).all()
        sess.close()


@pytest.mark.parametrize("max_batch", [1, 3, 16])
@pytest.mark.parametrize("tag", ["p10_s4_160x120", "p11_p2_120x68"])
def test_adaptive_session_ends_at_the_one_shot_image(pkg, orc, ctx, golden, tag, max_batch):
    """Adaptive (4, 2, the median variance at n = 4: a mixed count map), 12 samples at most: all at once, doubling, one sample per
    pass give the bits and counts of rtu_render_frame_adaptive; every snapshot's counts are min(done, the final count), and its rgb
    and z are, bit for bit, the numpy mean of each pixel's first `count` sample images."""
    g = golden(tag)
    scene = g.scene(pkg)
    gi = tag in PATH_TAGS
    S = 12
    ctx.upload(scene)
    fr = frame(pkg, scene, g.width, g.height, S, gi)
    t = mixed_target(orc.sample_images(scene, g.width, g.height, S, 0, 4, gi=gi, threads=OT), 4)
    ad = pkg.adaptive_defaults(min_samples=4, increment=2, target_variance=t, max_batch=max_batch)
    want, want_counts, _ = ctx.render_adaptive(fr, ad)
    assert (want_counts == 4).any() and (want_counts > 4).any(), "the count map is not mixed"
    imgs = ctx.sample_images(fr, 0, S)
    for schedule in ([S], [1, 1, 2, 4, 4], [1] * S):
        sess = ctx.progressive(fr, ad)
        done = 0
        for n, (got, counts) in zip(schedule, drive(sess, schedule)):
            done += n
            assert np.array_equal(counts, np.minimum(want_counts, done)), "%s: counts after %d samples" % (tag, done)
            assert same_bits(got, prefix_mean_counts(imgs, counts)), "%s: snapshot after %d samples is not the mean at its counts" % (tag, done)
        assert sess.status() == (S, 0)
        assert same_bits(got, want) and np.array_equal(counts, want_counts), "%s max_batch %d: schedule %s differs" % (tag, max_batch, schedule)
        sess.close()


# ---- 3. isolation --------------------------------------------------------------------------------------------------------------
def test_other_renders_between_passes(pkg, ctx, golden):
    """Between the passes of a recipe P session: a recipe W frame, a one-shot recipe S frame and a second (adaptive recipe S) session on
    the same context. Each result equals its reference rendered alone; the first session still ends at its one-shot image."""
    g = golden("p11_p2_120x68")
    scene = g.scene(pkg)
    W, H = g.width, g.height
    ctx.upload(scene)
    fa = frame(pkg, scene, W, H, 6, True)
    fw = pkg.frame_setup(scene.desc.camera, W, H)
    fs = frame(pkg, scene, W, H, 5, False)
    ad = pkg.adaptive_defaults(min_samples=2, increment=1, target_variance=0.01)
    want_a, _ = ctx.render(fa)
    want_w, _ = ctx.render(fw)
    want_s, _ = ctx.render(fs)
    want_b, want_bc, _ = ctx.render_adaptive(fs, ad)
    a = ctx.progressive(fa)
    b = ctx.progressive(fs, ad)
    a.advance(1)
    got, _ = ctx.render(fw)
    assert same_bits(got, want_w), "recipe W frame between passes"
    a.advance(2)
    b.advance(3)
    got, _ = ctx.render(fs)
    assert same_bits(got, want_s), "one-shot recipe S frame between passes"
    a.advance(3)
    b.advance(2)
    got_b, counts_b = b.snapshot()
    got_a, _ = a.snapshot()
    assert same_bits(got_a, want_a), "the session was disturbed"
    assert same_bits(got_b, want_b) and np.array_equal(counts_b, want_bc), "the second session was disturbed"
    a.close()
    b.close()


# ---- 4. shards -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adaptive", [False, True])
def test_three_shards_assemble_to_one(pkg, ctx, golden, adaptive):
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    W, H, S = g.width - 3, g.height - 3, 8  # ragged: partial tiles
    ctx.upload(scene)
    ad = pkg.adaptive_defaults(min_samples=2, increment=1, target_variance=0.002) if adaptive else None
    one = ctx.progressive(frame(pkg, scene, W, H, S, False), ad)
    frames = [frame(pkg, scene, W, H, S, False, r, 3) for r in range(3)]
    three = [ctx.progressive(f, ad) for f in frames]
    for n in (1, 2, 5):
        one.advance(n)
        want, want_counts = one.snapshot()
        shards = []
        for s in three:
            s.advance(n)
            shards.append(s.snapshot())
        got = pkg.assemble([x[0] for x in shards], frames, H)
        counts = np.empty((H, W), np.uint8)
        for (_, c), f in zip(shards, frames):
            counts[pkg.shard_global_rows(f)] = c
        assert same_bits(got, want) and np.array_equal(counts, want_counts), "3 shards differ from one"
    for s in three + [one]:
        s.close()


# ---- 5. lifecycle and refusals ----------------------------------------------------------------------------------------------
def test_refusals(pkg, ctx, golden):
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    ctx.upload(scene)
    fr = frame(pkg, scene, g.width, g.height, 8, False)

    def refused(f, ad=None, code=pkg.RTU_ERR_ARG):
        with pytest.raises(pkg.RtuError) as e:
            ctx.progressive(f, ad)
        assert e.value.code == code

    bad = frame(pkg, scene, g.width, g.height, 0, False)
    refused(bad)  # samples == 0: recipe W has nothing to refine
    bad = frame(pkg, scene, g.width, g.height, 8, False)
    bad.gather_bounces = 2
    refused(bad)
    bad = frame(pkg, scene, g.width, g.height, 8, False)
    bad.collect_stats = 1
    refused(bad)
    refused(frame(pkg, scene, g.width, g.height, 300, False), pkg.adaptive_defaults())  # adaptive counts are bytes
    refused(fr, pkg.adaptive_defaults(min_samples=0))
    refused(fr, pkg.adaptive_defaults(max_batch=17))
    refused(fr, pkg.adaptive_defaults(target_variance=float("nan")))
    sess = ctx.progressive(fr)
    for call in (lambda: sess.snapshot(), lambda: sess.advance(0), lambda: sess.advance(9)):
        with pytest.raises(pkg.RtuError) as e:
            call()
        assert e.value.code == pkg.RTU_ERR_ARG
    assert sess.status() == (0, (g.width + 7) // 8 * ((g.height + 7) // 8))
    sess.advance(5)
    with pytest.raises(pkg.RtuError) as e:
        sess.advance(4)  # past S
    assert e.value.code == pkg.RTU_ERR_ARG
    assert sess.status()[0] == 5
    sess.close()


@pytest.mark.parametrize("how", ["upload", "update"])
def test_stale_after_a_new_scene(pkg, ctx, golden, how):
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    ctx.upload(scene)
    sess = ctx.progressive(frame(pkg, scene, g.width, g.height, 8, False))
    sess.advance(3)
    before, _ = sess.snapshot()
    if how == "upload":
        ctx.upload(scene)
    else:
        ctx.update(scene)
    with pytest.raises(pkg.RtuError) as e:
        sess.advance(1)
    assert e.value.code == pkg.RTU_ERR_STALE
    after, counts = sess.snapshot()
    assert same_bits(after, before) and (counts == 3).all(), "the snapshot changed with the scene"
    sess.close()


def test_cancel_keeps_the_session(pkg, ctx, golden):
    """A raised cancel flag: RTU_ERR_CANCELLED, done unchanged; lowered again, the session resumes to the one-shot bits."""
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    ctx.upload(scene)
    fr = frame(pkg, scene, g.width, g.height, 8, False)
    want, _ = ctx.render(fr)
    sess = ctx.progressive(fr)
    sess.advance(2)
    flag = ctypes.c_int(1)
    ctx.set_cancel(flag)
    try:
        with pytest.raises(pkg.RtuError) as e:
            sess.advance(4)
        assert e.value.code == pkg.RTU_ERR_CANCELLED
        assert sess.status()[0] == 2
        flag.value = 0
        sess.advance(6)
    finally:
        ctx.set_cancel(None)
    got, _ = sess.snapshot()
    assert same_bits(got, want)
    sess.close()


def test_calls_after_the_context_is_destroyed(pkg, golden):
    """rtu_destroy_context frees the device memory of a session still open (the library's live device bytes return to what they were
    before the context was made, with the session handle not yet freed); the handle then answers RTU_ERR_ARG until it is freed."""
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    gc.collect()  # (no handle of an earlier test may free its buffers in the middle of this one)
    live0 = pkg.hip.rtu_debug_device_bytes()
    c = pkg.Context(0)
    c.upload(scene)
    with_scene = pkg.hip.rtu_debug_device_bytes()
    sess = c.progressive(frame(pkg, scene, g.width, g.height, 4, False), pkg.adaptive_defaults(min_samples=2))
    pixels = g.width * g.height
    assert pkg.hip.rtu_debug_device_bytes() - with_scene >= pixels * (16 + 16 + 4 + 1), "the session's sums are not its own buffers"
    sess.advance(2)
    c.close()
    assert pkg.hip.rtu_debug_device_bytes() == live0, "device memory still held after rtu_destroy_context"
    for call in (lambda: sess.advance(1), lambda: sess.snapshot(), lambda: sess.status()):
        with pytest.raises(pkg.RtuError) as e:
            call()
        assert e.value.code == pkg.RTU_ERR_ARG
    sess.close()
    assert pkg.hip.rtu_debug_device_bytes() == live0


# ---- 6. a capacity retry in mid-session ---------------------------------------------------------------------------------------
GLASSROOM_SOFT = """<xml><scene>
  <object type="sphere" name="room" material="wall"><scale value="60"/></object>
  <object type="sphere" name="ball" material="glassmirror"><scale value="9"/><translate x="0" y="0" z="0"/></object>
  <material type="blinn" name="wall"><diffuse r="0.7" g="0.6" b="0.5"/><specular value="0.2"/><glossiness value="10"/></material>
  <material type="blinn" name="glassmirror"><diffuse r="0.1" g="0.1" b="0.1"/><specular value="0.8"/><glossiness value="60"/>
    <reflection value="0.4" glossiness="0.05"/><refraction index="1.4" value="0.7"/></material>
  <light type="ambient" name="a"><intensity value="0.3"/></light>
  <light type="point" name="p"><size value="2"/><intensity value="0.8"/><position x="10" y="-20" z="25"/></light>
</scene><camera><position x="0" y="-14" z="0"/><target x="0" y="0" z="0"/><up x="0" y="0" z="1"/><fov value="70"/>
  <width value="128"/><height value="96"/></camera></xml>"""


@pytest.mark.parametrize("gi", [False, True])
def test_capacity_retry_in_mid_session(pkg, ctx, tmp_path, gi):
    """The glass room (up to three child frames per pixel: more than a fresh context provisions), glossy and with a soft light, on a
    FRESH context: the first batch runs out of frame records and is rendered again before it is added. Every snapshot is still the
    mean of the sample images, and the end is the one-shot image. (An overflow in mid-session: test_overflow_reported_in_mid_session.)"""
    xml = tmp_path / "glassroom_soft.xml"
    xml.write_text(GLASSROOM_SOFT)
    scene = pkg.Scene.from_xml(str(xml))
    W, H, S = 128, 96, 12
    fr = frame(pkg, scene, W, H, S, gi)
    ctx.upload(scene)
    imgs = ctx.sample_images(fr, 0, S)
    want, _ = ctx.render(fr)
    c = pkg.Context(0)
    try:
        c.upload(scene)
        sess = c.progressive(fr)
        done = 0
        for n in (1, 3, 8):
            sess.advance(n)
            done += n
            got, _ = sess.snapshot()
            assert same_bits(got, prefix_mean(imgs, done)), "snapshot after %d samples" % done
        assert same_bits(got, want)
        sess.close()
    finally:
        c.close()


GLASSROOM = GLASSROOM_SOFT.replace('<reflection value="0.4" glossiness="0.05"/>', '<reflection value="0.4"/>').replace('<size value="2"/>', '')


@pytest.mark.parametrize("case", ["s", "s_adaptive", "p"])
def test_overflow_reported_in_mid_session(pkg, ctx, tmp_path, case):
    """An overflow at done > 0, forced: after two passes, a recipe W frame of the glass room at 1024 x 768 — far more frames than the
    context has grown to — is rendered asynchronously on the same context and its status is left unread. The report is sticky, so the
    next pass's first batch is reported incomplete: it is rendered again before it is added (adaptive: the step kernel skips it). A
    twin context that runs the same sequence and reads the status shows the W frame does overflow there. After the pass the report has
    been consumed, the snapshot is the mean of the sample images, and the session still ends at the one-shot image."""
    xml = tmp_path / "glassroom.xml"
    xml.write_text(GLASSROOM)
    scene = pkg.Scene.from_xml(str(xml))
    W, H, S = 128, 96, 12
    gi = case == "p"
    ad = pkg.adaptive_defaults(min_samples=4, increment=2, target_variance=0.0005) if case == "s_adaptive" else None  # (all live at done = 3)
    fr = frame(pkg, scene, W, H, S, gi)
    fw = pkg.frame_setup(scene.desc.camera, 1024, 768)
    ctx.upload(scene)
    imgs = ctx.sample_images(fr, 0, S)
    if ad is None:
        want, want_counts = ctx.render(fr)[0], None
    else:
        want, want_counts, _ = ctx.render_adaptive(fr, ad)

    def start(c):
        c.upload(scene)
        sess = c.progressive(fr, ad)
        sess.advance(1)
        sess.advance(2)
        d = pkg.hip.rtu_device_alloc(c._h, 1024 * 768 * 16)
        c.render_device(fw, d, None)
        return sess, d

    twin = pkg.Context(0)
    try:
        sess, d = start(twin)
        with pytest.raises(pkg.RtuError) as e:
            twin.frame_status()
        assert e.value.code == pkg.RTU_ERR_CAPACITY, "the recipe W frame did not overflow: nothing is tested"
        pkg.hip.rtu_device_free(twin._h, d)
        sess.close()
    finally:
        twin.close()
    c = pkg.Context(0)
    try:
        sess, d = start(c)
        assert sess.status()[1] > 0  # (a pass that traces nothing would leave the report to the caller)
        sess.advance(3)  # the first batch of this pass sees the W frame's report
        c.frame_status()  # consumed by the pass
        pkg.hip.rtu_device_free(c._h, d)
        got, counts = sess.snapshot()
        ref = prefix_mean(imgs, 6) if ad is None else prefix_mean_counts(imgs, counts)
        assert same_bits(got, ref), "the snapshot after the overflowed pass is not the mean of the sample images"
        sess.advance(S - 6)
        got, counts = sess.snapshot()
        assert same_bits(got, want), "the session does not end at the one-shot image"
        if want_counts is not None:
            assert np.array_equal(counts, want_counts)
        sess.close()
    finally:
        c.close()


# ---- 7. the drop-in -------------------------------------------------------------------------------------------------------------
def one_shot_pngs(pkg, scene, W, H, S, gather, ad, d):
    img = pkg.Image(W, H)
    paths = [str(d / n) for n in ("Result.png", "ZBuffer.png", "SampleCount.png")]
    devs = (ctypes.c_int * 1)(0)
    if ad is not None:
        job = pkg.host.rtu_begin_render_adaptive(scene._h, img._h, devs, 1, S, gather, ctypes.byref(ad), *[p.encode() for p in paths])
    else:
        job = pkg.host.rtu_begin_render_sampled(scene._h, img._h, devs, 1, S, paths[0].encode(), paths[1].encode()) if gather == 0 else \
            pkg.host.rtu_begin_render_paths(scene._h, img._h, devs, 1, S, paths[0].encode(), paths[1].encode())
    assert job
    assert pkg.host.rtu_render_wait(job) == 0, pkg.host.rtu_host_last_error()
    pkg.host.rtu_render_job_free(job)
    return [read_png(p) for p in paths[:3 if ad is not None else 2]]


@pytest.mark.parametrize("mode", ["fixed_p", "adaptive_s"])
def test_begin_render_progressive(pkg, golden, tmp_path, mode):
    """On one device and on {0, 0, 0}: on_pass once per pass of the default schedule (1, 1, 2, 4, 4 for 12 samples), the pixel counter
    at W * H from the first pass on, and the decoded PNGs equal a one-shot job's."""
    tag = "p11_p2_120x68" if mode == "fixed_p" else "p10_s4_160x120"
    g = golden(tag)
    scene = g.scene(pkg)
    W, H, S = g.width, g.height, 12
    gather = 4 if mode == "fixed_p" else 0
    ad = pkg.adaptive_defaults(min_samples=4, increment=2, target_variance=0.002) if mode == "adaptive_s" else None
    d0 = tmp_path / "oneshot"
    d0.mkdir()
    want = one_shot_pngs(pkg, scene, W, H, S, gather, ad, d0)
    for devices in ([0], [0, 0, 0]):
        img = pkg.Image(W, H)
        d = tmp_path / ("n%d" % len(devices))
        d.mkdir()
        paths = [str(d / n) for n in ("Result.png", "ZBuffer.png", "SampleCount.png")]
        calls = []
        job = pkg.ProgressiveJob(scene, img, devices, S, gather, ad, None,
                                 lambda done, k: calls.append((done, k, pkg.host.rtu_image_num_rendered(img._h))), *paths)
        assert job.wait() == 0, pkg.host.rtu_host_last_error()
        job.close()
        assert [c[:2] for c in calls] == [(1, 1), (2, 2), (4, 3), (8, 4), (12, 5)]
        assert all(c[2] == W * H for c in calls)
        got = [read_png(p) for p in paths[:len(want)]]
        for a, b, name in zip(got, want, ("Result", "ZBuffer", "SampleCount")):
            assert np.array_equal(a, b), "%s.png differs from the one-shot job's (%d devices)" % (name, len(devices))


def test_stop_from_on_pass_keeps_the_last_pass(pkg, golden, tmp_path):
    """rtu_stop_render from on_pass after pass 2 (2 samples): rtu_render_wait returns RTU_ERR_CANCELLED, the image and Result.png hold
    exactly the snapshot of a session after 1 + 1 samples."""
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    W, H, S = g.width, g.height, 16
    c = pkg.Context(0)
    try:
        c.upload(scene)
        sess = c.progressive(frame(pkg, scene, W, H, S, False))
        sess.advance(1)
        sess.advance(1)
        snap, _ = sess.snapshot()
        sess.close()
    finally:
        c.close()
    want = pkg.Image(W, H)
    want.fill(snap)
    img = pkg.Image(W, H)
    rp, zp = str(tmp_path / "Result.png"), str(tmp_path / "ZBuffer.png")
    holder = {}
    made = threading.Event()

    def on_pass(done, k):
        if k == 2:
            made.wait(60)  # (the job thread may reach pass 2 before the constructor has returned the handle)
            holder["job"].stop()

    holder["job"] = job = pkg.ProgressiveJob(scene, img, [0], S, 0, None, None, on_pass, rp, zp)
    made.set()
    assert job.wait() == pkg.RTU_ERR_CANCELLED
    job.close()
    assert np.array_equal(img.pixels(), want.pixels())
    assert same_bits(img.zbuffer(), want.zbuffer())
    assert np.array_equal(read_png(rp), want.pixels())
