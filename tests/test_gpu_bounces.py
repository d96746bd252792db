"""GPU: RtuFrameDesc.max_bounce at every value (0..5) against the oracle at the same depth.

max_bounce fixes how a launch sequence is shaped (levels = max_bounce + 1 rounds of k_trace / k_trace2(c) / k_consume /
k_combine, where k_tail may cut, when the SEL_A pass and the collection of children stop) and the bounce count packed into every
root frame record. What the context learns from a frame (the cut level of k_tail, the stage-2 list lengths, occupied tiles,
side mode) is keyed by the launch shape, not by the depth: a hint learned at one depth is what the next frame of another depth
starts from, and must render the same image or be declined and rendered again.

The oracle takes the depth through its test hook (tests/test_oracle_bounces.py pins that hook to the compiled reference). Every
bar is the one the depth-5 test of the same scene uses: check_against with its defaults for recipe W, test_gpu_sampled.check
for recipe S, test_paths_vs_oracle's for recipe P, test_gpu_adaptive_oracle's for adaptive frames — a shallower depth multiplies
fewer powf / expf terms than depth 5 does. Everything but the side-mode turntable renders at the tags' own small sizes (160x120
to 240x135): thousands of frames in level 1, two to a few hundred in the deepest levels, the regime in which k_tail, the idle
cooperative launches and the level loop make their decisions."""
import ctypes
import os

import numpy as np
import pytest

from bench import ORBIT_STEP_DEG, orbit_camera
from conftest import GOLDEN
from test_gpu_adaptive import mixed_target
from test_gpu_adaptive_oracle import borderline
from test_gpu_parity import RGB8_TOL, check_against
from test_gpu_sampled import check
from test_gpu_workloads import check_paths, render_settled, slot_launches
from test_oracle_bounces import FIXTURES, TABLE

pytestmark = pytest.mark.gpu

OT = 16  # oracle threads
DEPTH_TAGS = list(TABLE)  # p4, p13, p5, p7 (textured), mtl (textured, MultiMtl), teapot2
SEQUENCE = (5, 1, 5, 2, 0, 4, 3, 5, 1)  # every depth after a deeper and after a shallower one
HINT_TAGS = ["p4_240x135", "teapot2_240x135", "p7_200x150"]
NCAM = 4


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def frame_at(pkg, cam, W, H, k, coop=None, **kw):
    fr = pkg.frame_setup(cam, W, H, max_bounce=k, **kw)
    if coop is not None:
        fr.coop_threshold = coop
    return fr


def cameras(scene, n=NCAM):
    """n distinct cameras, the first the scene's own (the cameras of test_frames_in_flight_equal_single_frames)."""
    cams = []
    for i in range(n):
        cam = type(scene.desc.camera).from_buffer_copy(bytes(scene.desc.camera))
        cam.pos[0] += 0.37 * i
        cam.pos[2] += 0.11 * i * i
        cam.fov += 1.5 * i
        cams.append(cam)
    return cams


def batch(pkg, ctx, frames, rows, W):
    """One launch sequence of the frames (rendered again while the context reports that it must be): [n, rows, W, 4]."""
    n = len(frames)
    d = pkg.hip.rtu_device_alloc(ctx._h, n * rows * W * 16)
    assert d
    try:
        render_settled(pkg, ctx, frames, d)
        got = np.empty((n, rows, W, 4), np.float32)
        assert pkg.hip.rtu_copy_to_host(ctx._h, got.ctypes.data, d, got.nbytes) == 0
    finally:
        pkg.hip.rtu_device_free(ctx._h, d)
    return got


@pytest.fixture(scope="module")
def oracle_at(pkg, orc, golden):
    """(image, stats) of the oracle's recipe W at depth k, rendered once per (tag, k) and never written to."""
    cache = {}

    def get(tag, k):
        if (tag, k) not in cache:
            g = golden(tag)
            out, st = orc.render(g.scene(pkg), g.width, g.height, threads=OT, max_bounce=k)
            out.setflags(write=False)
            cache[(tag, k)] = (out, st)
        return cache[(tag, k)]
    return get


@pytest.fixture(scope="module")
def fresh_at(pkg, golden):
    """The fast variant's images of cameras(scene) at depth k from a context that has rendered nothing else: [NCAM, H, W, 4],
    the first of them that context's first frame. Once per (tag, k)."""
    cache = {}

    def get(tag, k):
        if (tag, k) not in cache:
            g = golden(tag)
            scene = g.scene(pkg)
            c = pkg.Context(0)
            try:
                c.upload(scene)
                imgs = np.stack([c.render(frame_at(pkg, cam, g.width, g.height, k))[0] for cam in cameras(scene)])
            finally:
                c.close()
            imgs.setflags(write=False)
            cache[(tag, k)] = imgs
        return cache[(tag, k)]
    return get


# ---- (a) every depth against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(6))
@pytest.mark.parametrize("tag", DEPTH_TAGS)
def test_every_depth_vs_oracle(pkg, orc, ctx, golden, oracle_at, tag, k):
    """The counting variant against the oracle at depth k (image and every counter); the fast variant under both stage-2 forms and
    the touched-bytes variant are the counting variant's image bit for bit. Where the compiled reference left a fixture at this
    depth, its z, its 8-bit image and its counters are compared too."""
    g = golden(tag)
    scene = g.scene(pkg)
    W, H, cam = g.width, g.height, scene.desc.camera
    ctx.upload(scene)
    cnt, gst = ctx.render(frame_at(pkg, cam, W, H, k, collect_stats=True), stats=True)
    cpu, cst = oracle_at(tag, k)
    check_against(cnt, cpu, orc)
    assert gst == cst, "depth %d: counters differ: device %s, oracle %s" % (k, gst, cst)
    assert gst["secondary_rays"] == TABLE[tag][0][k]
    for coop in (10 ** 9, 1):
        fast, _ = ctx.render(frame_at(pkg, cam, W, H, k, coop=coop))
        assert same_bits(fast, cnt), "depth %d: fast (coop_threshold %d) and counting variants differ" % (k, coop)
    touched, _ = ctx.render(frame_at(pkg, cam, W, H, k, collect_stats=2))
    assert same_bits(touched, fast), "depth %d: the touched-bytes frame differs from the fast one" % k
    fr, _ = ctx.frame_counts()
    assert not any(fr[k + 1:]), "depth %d: frames below the last level: %s" % (k, fr)
    if k in FIXTURES.get(tag, ()):
        f = np.load(os.path.join(GOLDEN, tag, "bounce%d.npz" % k))
        assert same_bits(cnt[..., 3], f["z"])
        g8, _, gz8 = orc.postprocess(cnt)
        assert np.array_equal(gz8, f["zbuffer_u8"])
        assert np.abs(g8.astype(np.int32) - f["result_u8"].astype(np.int32)).max() <= RGB8_TOL
        assert (gst["primary_hits"], gst["secondary_rays"], gst["shadow_rays"]) == (int(f["primary_hits"]), int(f["secondary"]), int(f["shadow"]))


def test_teapot2_saturates_at_depth_2(pkg, ctx, golden):
    """Depths 2..5 of teapot2 are one image while the rays still grow: 825, 978, 979, 980 secondary rays."""
    g = golden("teapot2_240x135")
    scene = g.scene(pkg)
    ctx.upload(scene)
    imgs, rays = {}, {}
    for k in range(1, 6):
        imgs[k], _ = ctx.render(frame_at(pkg, scene.desc.camera, g.width, g.height, k))
        _, st = ctx.render(frame_at(pkg, scene.desc.camera, g.width, g.height, k, collect_stats=True), stats=True)
        rays[k] = st["secondary_rays"]
    assert not same_bits(imgs[1], imgs[2])
    for k in (3, 4, 5):
        assert same_bits(imgs[k], imgs[2]), "depth %d is not the depth-2 image" % k
    assert [rays[k] for k in (2, 3, 4, 5)] == [825, 978, 979, 980]


# ---- (b) hints learned at another depth ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", HINT_TAGS)
def test_hints_learned_at_another_depth_single_frames(pkg, golden, fresh_at, tag):
    """One context, one launch shape, the depths of SEQUENCE through rtu_render_frame: every image is the image a fresh context
    renders at that depth, bit for bit, and the context reports no error."""
    g = golden(tag)
    scene = g.scene(pkg)
    c = pkg.Context(0)
    try:
        c.upload(scene)
        for i, k in enumerate(SEQUENCE):
            got, _ = c.render(frame_at(pkg, scene.desc.camera, g.width, g.height, k))
            assert same_bits(got, fresh_at(tag, k)[0]), "frame %d of the sequence (depth %d, after %s) is not a fresh context's" % (i, k, SEQUENCE[:i])
            c.frame_status()
            fr, _ = c.frame_counts()
            assert not any(fr[k + 1:]), "frame %d (depth %d): frames below the last level: %s" % (i, k, fr)
    finally:
        c.close()
    for k in range(1, 6):
        if tag != "teapot2_240x135" or k <= 2:
            assert not same_bits(fresh_at(tag, k)[0], fresh_at(tag, k - 1)[0]), "depths %d and %d do not differ" % (k - 1, k)


@pytest.mark.parametrize("tag", HINT_TAGS)
def test_hints_learned_at_another_depth_batches(pkg, golden, fresh_at, tag):
    """The same sequence as launch sequences of four frames with distinct cameras (rtu_render_frames_device)."""
    g = golden(tag)
    scene = g.scene(pkg)
    W, H = g.width, g.height
    c = pkg.Context(0)
    try:
        c.upload(scene)
        for i, k in enumerate(SEQUENCE):
            got = batch(pkg, c, [frame_at(pkg, cam, W, H, k) for cam in cameras(scene)], H, W)
            want = fresh_at(tag, k)
            for j in range(NCAM):
                assert same_bits(got[j], want[j]), "batch %d (depth %d, after %s), frame %d is not a fresh context's" % (i, k, SEQUENCE[:i], j)
            c.frame_status()
            c.frame_counts()
    finally:
        c.close()


# ---- (c) the tail at every cut -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("tag", ["p4_240x135", "p13_200x150", "p7_200x150"])
def test_tail_kernel_any_cut_level_at_depth(pkg, orc, ctx, golden, oracle_at, tag, k):
    """test_tail_kernel_any_cut_level at depths 1..4: levels >= `level` evaluated by k_tail, for every level 1..5 — cuts at or
    below the last level (k + 1 <= level) leave nothing to k_tail — give the uncut image bit for bit."""
    g = golden(tag)
    scene = g.scene(pkg)
    ctx.upload(scene)
    fr = frame_at(pkg, scene.desc.camera, g.width, g.height, k)
    assert pkg.hip.rtu_debug_tail_from(ctx._h, 6) == 0
    ref, _ = ctx.render(fr)
    check_against(ref, oracle_at(tag, k)[0], orc)
    for level in (1, 2, 3, 4, 5):
        assert pkg.hip.rtu_debug_tail_from(ctx._h, level) == 0
        tail, _ = ctx.render(fr)
        assert same_bits(ref, tail), "depth %d: a cut at level %d changes the image" % (k, level)


# ---- (d) batches and shards ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("tag", ["p4_240x135", "p7_200x150"])
def test_frames_in_flight_equal_single_frames_at_depth(pkg, ctx, golden, tag, k):
    g = golden(tag)
    scene = g.scene(pkg)
    W, H = g.width, g.height
    ctx.upload(scene)
    cams = cameras(scene)
    singles = [ctx.render(frame_at(pkg, cam, W, H, k))[0] for cam in cams]
    assert not same_bits(singles[0], singles[1])
    deeper, _ = ctx.render(frame_at(pkg, cams[0], W, H, k + 1))
    assert not same_bits(singles[0], deeper), "the depth does not show in this frame"
    for stats in (0, 1):
        got = batch(pkg, ctx, [frame_at(pkg, cam, W, H, k, collect_stats=stats) for cam in cams], H, W)
        for j in range(NCAM):
            assert same_bits(got[j], singles[j]), "depth %d: frame %d of the batch differs (stats=%d)" % (k, j, stats)


@pytest.mark.parametrize("tag", ["p4_240x135", "p7_200x150"])
def test_three_shards_assemble_at_depth_2(pkg, orc, ctx, golden, oracle_at, tag):
    g = golden(tag)
    scene = g.scene(pkg)
    W, H, k = g.width, g.height, 2
    ctx.upload(scene)
    cams = cameras(scene)
    one = [ctx.render(frame_at(pkg, cam, W, H, k))[0] for cam in cams]
    check_against(one[0], oracle_at(tag, k)[0], orc)
    parts, frames = [], []
    for r in range(3):
        fr = frame_at(pkg, cams[0], W, H, k, shard_rank=r, shard_count=3)
        parts.append(ctx.render(fr)[0])
        frames.append(fr)
    assert same_bits(pkg.assemble(parts, frames, H), one[0]), "three single-frame shards differ from one"
    got = []
    for r in range(3):  # and as launch sequences of four frames per shard
        frs = [frame_at(pkg, cam, W, H, k, shard_rank=r, shard_count=3) for cam in cams]
        got.append(batch(pkg, ctx, frs, pkg.shard_rows(frs[0]), W))
    for j in range(NCAM):
        frs = [frame_at(pkg, cams[j], W, H, k, shard_rank=r, shard_count=3) for r in range(3)]
        assert same_bits(pkg.assemble([got[r][j] for r in range(3)], frs, H), one[j]), "frame %d: three batch shards differ from one" % j


@pytest.mark.parametrize("k", [1, 2])
def test_turntable_side_mode_at_depth(pkg, orc, ctx, golden, k):
    """test_turntable_side_mode's launches at depth k: one 20-frame launch sequence of the teapot2 turntable. From the second launch
    of the shape on, stage 2 of the primary phase runs in side mode (k_tail on the side arrays from level 0, with levels = k + 1) —
    a touched-bytes launch of the same shape shows k_tail(side) launched, and none under rtu_debug_flags 8192 —; both render every
    frame as rtu_render_frame does alone, and as the oracle does at that camera and depth.
    (The one test of this module at 1920x1080: side mode is taken for stage-2 lists beyond the default threshold of 70000 rays,
    which 20 frames of 240x135 do not defer — measured: no k_tail(side) launch there, even with a threshold of 1.)"""
    g = golden("teapot2_1080")
    scene = g.scene(pkg)
    W, H, B = g.width, g.height, 20
    cams = [orbit_camera(scene.desc.camera, ORBIT_STEP_DEG * j) for j in range(B)]
    ctx.upload(scene)
    d = pkg.hip.rtu_device_alloc(ctx._h, B * W * H * 16)
    got = np.empty((B, H, W, 4), np.float32)
    outs = {}
    try:
        for flags in (0, 8192):
            assert pkg.hip.rtu_debug_flags(ctx._h, flags) == 0
            for _ in range(2):
                render_settled(pkg, ctx, [frame_at(pkg, c, W, H, k) for c in cams], d)
            render_settled(pkg, ctx, [frame_at(pkg, c, W, H, k, collect_stats=2) for c in cams], d)
            side = slot_launches(pkg, ctx, "k_tail(side)")
            assert (side >= 1) if flags == 0 else (side == 0), "flags %d: %d k_tail(side) launches" % (flags, side)
            assert pkg.hip.rtu_copy_to_host(ctx._h, got.ctypes.data, d, got.nbytes) == 0
            outs[flags] = got.copy()
    finally:
        pkg.hip.rtu_debug_flags(ctx._h, 0)
        pkg.hip.rtu_device_free(ctx._h, d)
    assert same_bits(outs[0], outs[8192]), "side mode changes the images"
    for j in range(B):
        single, _ = ctx.render(frame_at(pkg, cams[j], W, H, k))
        assert same_bits(outs[0][j], single), "frame %d of the batch is not the single frame" % j
    shallower, _ = ctx.render(frame_at(pkg, cams[0], W, H, k - 1))  # (teapot2 saturates at depth 2: compare downwards)
    assert not same_bits(shallower, outs[0][0]), "the depth does not show in this frame"
    for j in (0, 19):
        old = type(cams[j]).from_buffer_copy(scene.desc.camera)
        scene.desc.camera = cams[j]
        try:
            cpu, _ = orc.render(scene, W, H, threads=OT, max_bounce=k)
        finally:
            scene.desc.camera = old
        check_against(outs[0][j], cpu, orc)


def test_a_batch_of_mixed_depths_is_refused(pkg, ctx, golden):
    g = golden("p4_240x135")
    scene = g.scene(pkg)
    W, H = g.width, g.height
    ctx.upload(scene)
    cams = cameras(scene, 2)
    before = [ctx.render(frame_at(pkg, cam, W, H, 3))[0] for cam in cams]
    d = pkg.hip.rtu_device_alloc(ctx._h, 2 * W * H * 16)
    try:
        for ka, kb in ((3, 2), (2, 3), (5, 0)):
            arr = (pkg.RtuFrameDesc * 2)(frame_at(pkg, cams[0], W, H, ka), frame_at(pkg, cams[1], W, H, kb))
            assert pkg.hip.rtu_render_frames_device(ctx._h, arr, 2, d, None) == pkg.RTU_ERR_ARG
        ctx.frame_status()  # nothing was queued, nothing is reported
    finally:
        pkg.hip.rtu_device_free(ctx._h, d)
    got = batch(pkg, ctx, [frame_at(pkg, cam, W, H, 3) for cam in cams], H, W)
    assert same_bits(got[0], before[0]) and same_bits(got[1], before[1]), "the context renders otherwise after the refusal"


# ---- (e) sampled, path-traced, adaptive and progressive frames -------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
def test_recipe_s_at_depth(pkg, orc, ctx, golden, k):
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    W, H, spp = g.width, g.height, 2
    cpu, cst = orc.render_samples(scene, W, H, spp, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=OT, max_bounce=k)
    deep, _ = orc.render_samples(scene, W, H, spp, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=OT, max_bounce=k + 1)
    assert not same_bits(cpu, deep), "the depth does not show in this frame"
    ctx.upload(scene)
    cam = scene.desc.camera
    fast, _ = ctx.render(frame_at(pkg, cam, W, H, k, samples=spp))
    check(fast, cpu, orc, spp, "p10 depth %d" % k)
    for coop in (1 << 30, 1):  # both stage-2 forms
        again, _ = ctx.render(frame_at(pkg, cam, W, H, k, samples=spp, coop=coop))
        assert same_bits(again, fast), "depth %d: the stage-2 form (coop_threshold %d) changes the image" % (k, coop)
    cnt, gst = ctx.render(frame_at(pkg, cam, W, H, k, samples=spp, collect_stats=True), stats=True)
    assert same_bits(cnt, fast), "fast and counting variants differ"
    assert gst == cst, "depth %d: counters differ: device %s, oracle %s" % (k, gst, cst)


def test_recipe_p_at_depth_2(pkg, orc, ctx, golden):
    """Recipe P: both Shade() calls of the pixel and both of every gather bounce receive max_bounce (k_gi_roots)."""
    g = golden("p13_p2_96x72")
    scene = g.scene(pkg)
    W, H, spp, k = g.width, g.height, 2, 2
    cpu, cst = orc.render_paths(scene, W, H, spp, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=OT, max_bounce=k)
    full, _ = orc.render_paths(scene, W, H, spp, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=OT)
    assert not same_bits(cpu, full), "the depth does not show in this frame"
    ctx.upload(scene)
    gpu, _ = ctx.render(frame_at(pkg, scene.desc.camera, W, H, k, samples=spp, gather_bounces=4))
    check_paths(gpu, cpu, orc, "p13 recipe P depth 2")
    cnt, gst = ctx.render(frame_at(pkg, scene.desc.camera, W, H, k, samples=spp, gather_bounces=4, collect_stats=True), stats=True)
    assert same_bits(cnt, gpu), "fast and counting variants differ"
    assert gst == cst, "counters differ: device %s, oracle %s" % (gst, cst)


def test_adaptive_frame_at_depth_2(pkg, orc, ctx, golden):
    """test_gpu_adaptive_oracle.test_golden_scene's median4 rule (4, 2, the median variance at n = 4) and its bars (compare) on p10
    at depth 2: counts equal the oracle's except at borderline pixels (0.1 % at most), the image is the oracle's mean of each
    pixel's first n samples at the device's count n within test_gpu_sampled.check."""
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    W, H, spp, k = g.width, g.height, 16, 2
    t = mixed_target(orc.sample_images(scene, W, H, spp, 0, 4, threads=OT, max_bounce=k), 4)
    ad = pkg.adaptive_defaults(min_samples=4, increment=2, target_variance=t)
    ctx.upload(scene)
    got, counts, _ = ctx.render_adaptive(frame_at(pkg, scene.desc.camera, W, H, k, samples=spp), ad)
    assert (counts == 4).any() and (counts > 4).any(), "the count map is not mixed"
    cpu, ocounts, margin, _ = orc.render_adaptive(scene, W, H, spp, 4, 2, float(t), counts_in=counts, threads=OT, max_bounce=k)
    border = borderline(margin, float(t))
    differ = counts != ocounts
    bad = differ & ~border
    assert not bad.any(), "%d pixels stop elsewhere than the oracle, clear of the target" % int(bad.sum())
    assert differ.sum() <= 1e-3 * differ.size, "%d borderline pixels stop elsewhere" % int(differ.sum())
    check(got, cpu, orc, spp, "p10 adaptive depth 2")
    deep, dcounts, _, _ = orc.render_adaptive(scene, W, H, spp, 4, 2, float(t), threads=OT)
    assert not same_bits(deep, cpu) or not np.array_equal(dcounts, ocounts), "the depth does not show in this frame"


def test_progressive_session_at_depth_2(pkg, ctx, golden):
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    W, H, S, k = g.width, g.height, 8, 2
    ctx.upload(scene)
    fr = frame_at(pkg, scene.desc.camera, W, H, k, samples=S)
    want, _ = ctx.render(fr)
    full, _ = ctx.render(frame_at(pkg, scene.desc.camera, W, H, 5, samples=S))
    assert not same_bits(want, full), "the depth does not show in this frame"
    sess = ctx.progressive(fr)
    try:
        for n in (1, 1, 2, 4):
            sess.advance(n)
        assert sess.status() == (S, 0)
        got, counts = sess.snapshot()
    finally:
        sess.close()
    assert same_bits(got, want), "the session at depth 2 does not end at the fixed frame of depth 2"
    assert (counts == S).all()


# ---- (f) the contract ----------------------------------------------------------------------------------------------------------
def test_max_bounce_out_of_range_is_refused_everywhere(pkg, ctx, golden):
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    W, H = 32, 24
    ctx.upload(scene)
    cam = scene.desc.camera
    out = np.empty((H, W, 4), np.float32)
    counts = np.empty((H, W), np.uint8)
    ad = pkg.adaptive_defaults()
    d = pkg.hip.rtu_device_alloc(ctx._h, 2 * W * H * 16)
    try:
        for bad in (-1, 6):
            s = frame_at(pkg, cam, W, H, bad, samples=2)
            assert pkg.hip.rtu_render_frame(ctx._h, ctypes.byref(s), out.ctypes.data, None) == pkg.RTU_ERR_ARG
            assert pkg.hip.rtu_render_frame_device(ctx._h, ctypes.byref(s), d, None) == pkg.RTU_ERR_ARG
            assert pkg.hip.rtu_render_frame_adaptive(ctx._h, ctypes.byref(s), ctypes.byref(ad), out.ctypes.data, counts.ctypes.data, None) == pkg.RTU_ERR_ARG
            assert pkg.hip.rtu_render_frame_adaptive_device(ctx._h, ctypes.byref(s), ctypes.byref(ad), d, None, None) == pkg.RTU_ERR_ARG
            for adaptive in (None, ctypes.byref(ad)):
                err = ctypes.c_int(0)
                assert not pkg.hip.rtu_progressive_begin(ctx._h, ctypes.byref(s), adaptive, ctypes.byref(err))
                assert err.value == pkg.RTU_ERR_ARG
        for k in (0, 5):  # the ends of the range are inside it
            s = frame_at(pkg, cam, W, H, k, samples=2)
            assert pkg.hip.rtu_render_frame(ctx._h, ctypes.byref(s), out.ctypes.data, None) == 0
        plain = golden("p4_240x135").scene(pkg)  # recipe W: a deterministic scene
        ctx.upload(plain)
        for bad in (-1, 6):
            w = frame_at(pkg, plain.desc.camera, W, H, bad)
            assert pkg.hip.rtu_render_frame(ctx._h, ctypes.byref(w), out.ctypes.data, None) == pkg.RTU_ERR_ARG
            assert pkg.hip.rtu_render_frame_device(ctx._h, ctypes.byref(w), d, None) == pkg.RTU_ERR_ARG
            arr = (pkg.RtuFrameDesc * 2)(w, w)
            assert pkg.hip.rtu_render_frames_device(ctx._h, arr, 2, d, None) == pkg.RTU_ERR_ARG
        ctx.frame_status()
    finally:
        pkg.hip.rtu_device_free(ctx._h, d)


def test_multi_context_at_depth_2(pkg, orc, ctx, golden, oracle_at):
    g = golden("p4_240x135")
    scene = g.scene(pkg)
    W, H, k = g.width, g.height, 2
    ctx.upload(scene)
    ref, _ = ctx.render(frame_at(pkg, scene.desc.camera, W, H, k))
    check_against(ref, oracle_at("p4_240x135", k)[0], orc)
    m = pkg.MultiContext([0, 0, 0])
    try:
        m.upload(scene)
        img = m.render(frame_at(pkg, scene.desc.camera, W, H, k))
    finally:
        m.close()
    assert same_bits(img, ref)


def test_depth_2_after_a_material_update(pkg, golden):
    """test_feature_flags_follow_the_update's edit: the teapot's material turned into a mirror and back by rtu_update_scene. A frame
    at depth 2 after each step equals a fresh upload's (with the mirror, mesh hits have children: the depth shows on the teapot)."""
    from test_gpu_scene_update import materials, mesh_nodes, nodes
    g = golden("teapot2_240x135")
    scene = g.scene(pkg)
    W, H, k = g.width, g.height, 2

    def fresh():
        c = pkg.Context(0)
        try:
            c.upload(scene)
            return [c.render(frame_at(pkg, scene.desc.camera, W, H, d))[0] for d in (k, k + 1)]
        finally:
            c.close()
    a = pkg.Context(0)
    try:
        a.upload(scene)
        plain = fresh()
        first, _ = a.render(frame_at(pkg, scene.desc.camera, W, H, k))
        assert same_bits(first, plain[0])
        m = materials(scene)[nodes(scene)[mesh_nodes(scene)[0]].material_id]
        old = [m.reflection[i] for i in range(3)]
        m.reflection[0] = m.reflection[1] = m.reflection[2] = 0.5
        a.update(scene)
        mirror = fresh()
        assert not same_bits(mirror[0], plain[0]) and not same_bits(mirror[0], mirror[1])
        got, _ = a.render(frame_at(pkg, scene.desc.camera, W, H, k))
        assert same_bits(got, mirror[0]), "depth 2 after the update to a mirror is not a fresh upload's"
        for i in range(3):
            m.reflection[i] = old[i]
        a.update(scene)
        got, _ = a.render(frame_at(pkg, scene.desc.camera, W, H, k))
        assert same_bits(got, plain[0]), "depth 2 after the update back is not a fresh upload's"
    finally:
        a.close()
