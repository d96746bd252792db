"""GPU: the configurations bench.py times and BASELINE.md names, frame by frame against the CPU oracle.

A. The headline turntable (bench.py defaults: teapot2_1080, 32 frames per launch sequence, each with its own camera
   bench.orbit_camera 2 degrees apart, two contexts alternating on two streams with two sequences in flight): every frame of
   every sequence against the oracle at its camera, the counting variant's counters at every camera; side mode (stage 2 of
   the primary phase beside the recursion levels) shown to be taken at 20 frames; 128 distinct cameras in one launch sequence.
B. Frames with more samples than one launch sequence holds (render_sampled: batches of min(16, 2^25 / pixels) samples,
   each at its own sample offset, accumulated in sample order): recipes S and P across batch boundaries, batches shorter
   than 16, config 5 itself, accumulators of an earlier frame, and the capacity retry with counters.

Bars as in test_gpu_parity / test_gpu_sampled: float z bit-exact, z-image equal, 8-bit RGB within one level, NaN colours at
the same pixels, linear RGB to 2e-5 (recipe W) / 2e-4 (recipe S) / 1e-3 of the value (recipe P), counters equal."""
import ctypes
import math

import numpy as np
import pytest

from bench import ORBIT_STEP_DEG, orbit_camera
from test_gpu_parity import RGB8_TOL, check_against
from test_gpu_sampled import check, render_gpu, render_paths_gpu

pytestmark = pytest.mark.gpu

OT = 16  # oracle threads


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def at_camera(scene, cam):
    """The scene with its camera replaced (what the oracle renders from); returns the camera it had."""
    old = type(cam).from_buffer_copy(scene.desc.camera)
    scene.desc.camera = cam
    return old


def oracle_w(orc, scene, cam, W, H, row0=0, nrows=None):
    old = at_camera(scene, cam)
    try:
        return orc.render(scene, W, H, threads=OT, row0=row0, nrows=nrows)
    finally:
        scene.desc.camera = old


def render_settled(pkg, ctx, frames, d, stream=None):
    """One launch sequence of len(frames) frames into d, repeated while a recursion level runs out of frame records."""
    for attempt in range(8):
        ctx.render_frames_device(frames, d, stream)
        try:
            ctx.frame_status()
            return
        except pkg.RtuError as e:
            if e.code != pkg.RTU_ERR_CAPACITY or attempt == 7:
                raise


def slot_launches(pkg, ctx, name):
    """Launches of one kernel slot since the counters were last zeroed (touched-bytes mode)."""
    arr = (ctypes.c_uint32 * pkg.KERNEL_SLOTS)()
    n = pkg.hip.rtu_get_touched_launches(ctx._h, arr, pkg.KERNEL_SLOTS)
    names = [pkg.hip.rtu_kernel_slot_name(k).decode() for k in range(n)]
    return int(arr[names.index(name)])


def check_paths(gpu, cpu, orc, what):
    """Recipe P's bar (test_paths_vs_oracle): z bit-exact, z-image equal, 8-bit RGB within one level, linear RGB to 1e-3 of the value."""
    assert np.array_equal(gpu[..., 3].view(np.uint32), cpu[..., 3].view(np.uint32)), what + ": z differs"
    g8, _, gz8 = orc.postprocess(gpu)
    c8, _, cz8 = orc.postprocess(cpu)
    assert np.array_equal(gz8, cz8), what + ": z-image differs"
    d8 = np.abs(g8.astype(np.int32) - c8.astype(np.int32))
    assert d8.max() <= RGB8_TOL, "%s: 8-bit RGB differs by %d levels at %d pixels" % (what, d8.max(), (d8 > RGB8_TOL).sum())
    d = np.abs(gpu[..., :3].astype(np.float64) - cpu[..., :3].astype(np.float64))
    assert (d / np.maximum(np.abs(cpu[..., :3]), 1e-2)).max() < 1e-3, what + ": linear RGB differs"


# ---- A. the benchmarked turntable ---------------------------------------------------------------------------
def test_benchmarked_turntable_frame_by_frame(pkg, orc, golden):
    """bench.py's headline launch sequences as bench.py queues them: two contexts, each on a stream of its own and told that two
    sequences are in flight, warmed up until frame_status is clean, then three 32-frame sequences per context queued alternately
    before one frame_status each. Every frame of every sequence is the same bits and equals the oracle at its turntable camera.
    A fast and a touched-bytes launch of the same shape render the same images with and without rtu_debug_flags 8192 (no
    side mode: no k_tail(side) launch). The counting variant's counters equal the oracle's at each of the 32 cameras."""
    import torch
    g = golden("teapot2_1080")
    scene = g.scene(pkg)
    W, H, B, C, SEQ = g.width, g.height, 32, 2, 3
    cams = [orbit_camera(scene.desc.camera, ORBIT_STEP_DEG * j) for j in range(B)]
    ctxs, bufs, ref_d = [], [], None
    try:
        for _ in range(C):
            c = pkg.Context(0)
            ctxs.append(c)
            c.upload(scene)
            assert pkg.hip.rtu_set_sequences_in_flight(c._h, C) == 0
        streams = [torch.cuda.Stream(device=0) for _ in range(C)]
        bufs = [torch.empty(B * H * W * 4, dtype=torch.float32, device="cuda:0") for _ in range(C * SEQ)]
        fast = [pkg.frame_setup(cam, W, H) for cam in cams]
        touch = [pkg.frame_setup(cam, W, H, collect_stats=2) for cam in cams]

        def queue(k, frames, buf):
            ctxs[k].render_frames_device(frames, buf.data_ptr(), streams[k].cuda_stream)

        def settle(frames):
            for attempt in range(13):  # (bench.settle)
                for k in range(C):
                    queue(k, frames, bufs[k])
                clean = True
                for c in ctxs:
                    try:
                        c.frame_status()
                    except pkg.RtuError as e:
                        if e.code != pkg.RTU_ERR_CAPACITY or attempt == 12:
                            raise
                        clean = False
                if clean:
                    return

        def same(buf, want):
            torch.cuda.synchronize()
            return torch.equal(buf.view(torch.int32), want.view(torch.int32))

        settle(fast)
        for s in range(SEQ):
            for k in range(C):
                queue(k, fast, bufs[s * C + k])
        for c in ctxs:
            c.frame_status()
        ref_d = bufs[0].clone()
        for s in range(1, len(bufs)):
            assert same(bufs[s], ref_d), "sequence %d of context %d differs from the first" % (s // C, s % C)
        ref = ref_d.view(B, H, W, 4).cpu().numpy()
        ostats = []
        for j, cam in enumerate(cams):
            cpu, cst = oracle_w(orc, scene, cam, W, H)
            ostats.append(cst)
            try:
                check_against(ref[j], cpu, orc)
            except AssertionError as e:
                raise AssertionError("turntable frame %d: %s" % (j, e))
        # the images do not depend on where stage 2 of the primary phase runs. (32 turntable frames are NOT in side mode: from frame
        # 28 on, the glass sphere seen through the teapot's box makes stage 2 append more than the 256 frames side mode takes;
        # test_turntable_side_mode below shows the mode at the 20-frame sequence of bench.py --steps 20)
        for flags in (0, 8192):
            for c in ctxs:
                assert pkg.hip.rtu_debug_flags(c._h, flags) == 0
            if flags:
                settle(fast)  # (without side mode the main level arrays take stage 2's frames)
            for k, c in enumerate(ctxs):
                queue(k, fast, bufs[k])
                c.frame_status()
                queue(k, touch, bufs[C + k])
                c.frame_status()
                if flags:
                    assert slot_launches(pkg, c, "k_tail(side)") == 0, "context %d: side mode taken under rtu_debug_flags 8192" % k
                assert same(bufs[k], ref_d) and same(bufs[C + k], ref_d), "flags %d, context %d: images differ" % (flags, k)
        for c in ctxs:
            pkg.hip.rtu_debug_flags(c._h, 0)
        # the numerator of Grays/s: the counting variant at every turntable camera
        for j, cam in enumerate(cams):
            img, gst = ctxs[0].render(pkg.frame_setup(cam, W, H, collect_stats=True), stats=True)
            assert gst == ostats[j], "camera %d: counters differ" % j
            assert np.array_equal(img.view(np.uint32), ref[j].view(np.uint32)), "camera %d: counting variant differs" % j
    finally:
        bufs = ref_d = None
        for c in ctxs:
            c.close()
        torch.cuda.empty_cache()


def test_turntable_side_mode(pkg, orc, ctx, golden):
    """bench.py --steps 20 (one 20-frame launch sequence of the turntable, the configuration of the recorded benchmarks): from the
    second launch of the shape on, stage 2 of the primary phase runs in side mode — a touched-bytes launch of the same shape shows
    k_tail(side) launched —, and under rtu_debug_flags 8192 it does not; both render every frame as the oracle does."""
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
                render_settled(pkg, ctx, [pkg.frame_setup(c, W, H) for c in cams], d)
            render_settled(pkg, ctx, [pkg.frame_setup(c, W, H, collect_stats=2) for c in cams], d)
            side = slot_launches(pkg, ctx, "k_tail(side)")
            assert (side >= 1) if flags == 0 else (side == 0), "flags %d: %d k_tail(side) launches" % (flags, side)
            assert pkg.hip.rtu_copy_to_host(ctx._h, got.ctypes.data, d, got.nbytes) == 0
            outs[flags] = got.copy()
    finally:
        pkg.hip.rtu_debug_flags(ctx._h, 0)
        pkg.hip.rtu_device_free(ctx._h, d)
    assert np.array_equal(outs[0].view(np.uint32), outs[8192].view(np.uint32)), "side mode changes the images"
    for j, cam in enumerate(cams):
        cpu, _ = oracle_w(orc, scene, cam, W, H)
        try:
            check_against(outs[0][j], cpu, orc)
        except AssertionError as e:
            raise AssertionError("frame %d: %s" % (j, e))


@pytest.mark.parametrize("tag,size,n", [("teapot2_240x135", None, 128), ("p4_240x135", None, 128), ("p11_240x135", None, 128),
                                        ("teapot2_240x135", (203, 117), 40)])
def test_many_distinct_cameras_in_one_batch(pkg, orc, ctx, golden, tag, size, n):
    """One launch sequence of up to RTU_MAX_FRAMES_IN_FLIGHT frames, the turntable 2 degrees apart (128 frames: most of the way
    round), every frame against the oracle at its camera; a ragged size (not a multiple of 8) with 40 frames."""
    g = golden(tag)
    scene = g.scene(pkg)
    W, H = size or (g.width, g.height)
    ctx.upload(scene)
    cams = [orbit_camera(scene.desc.camera, ORBIT_STEP_DEG * j) for j in range(n)]
    d = pkg.hip.rtu_device_alloc(ctx._h, n * W * H * 16)
    try:
        render_settled(pkg, ctx, [pkg.frame_setup(c, W, H) for c in cams], d)
        got = np.empty((n, H, W, 4), np.float32)
        assert pkg.hip.rtu_copy_to_host(ctx._h, got.ctypes.data, d, got.nbytes) == 0
    finally:
        pkg.hip.rtu_device_free(ctx._h, d)
    for j, cam in enumerate(cams):
        cpu, _ = oracle_w(orc, scene, cam, W, H)
        try:
            check_against(got[j], cpu, orc)
        except AssertionError as e:
            raise AssertionError("frame %d of %d: %s" % (j, n, e))


# ---- B. many-sample frames across launch-sequence batches ---------------------------------------------------
SPPS = [16, 17, 33, 64]


@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("tag", ["p10_s4_160x120", "teapot1_s2_160x90"])
def test_sampled_across_batches(pkg, orc, ctx, golden, tag, spp):
    """Recipe S with 1 to 4 batches of 16 samples: the fast variant, the counting variant's counters and 3 shards against
    the oracle; a touched-bytes frame launches k_primary once per batch."""
    g = golden(tag)
    scene = g.scene(pkg)
    W, H = g.width, g.height
    cpu, cst = orc.render_samples(scene, W, H, spp, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=OT)
    fast, _ = render_gpu(pkg, ctx, scene, W, H, spp)
    check(fast, cpu, orc, spp, "%s %d spp" % (tag, spp))
    cnt, gst = render_gpu(pkg, ctx, scene, W, H, spp, stats=True)
    assert np.array_equal(cnt.view(np.uint32), fast.view(np.uint32)), "fast and counting variants differ"
    assert gst == cst, "counters differ"
    three, _ = render_gpu(pkg, ctx, scene, W, H, spp, shard_count=3)
    assert np.array_equal(three.view(np.uint32), fast.view(np.uint32)), "3 shards differ from one"
    img, _ = ctx.render(pkg.frame_setup(scene.desc.camera, W, H, collect_stats=2, samples=spp))
    assert np.array_equal(img.view(np.uint32), fast.view(np.uint32)), "touched-bytes frame differs"
    assert slot_launches(pkg, ctx, "k_primary") == math.ceil(spp / 16)


def _touched_primary_launches(pkg, ctx, scene, W, H, spp):
    img, _ = ctx.render(pkg.frame_setup(scene.desc.camera, W, H, collect_stats=2, samples=spp, gather_bounces=4))
    return img, slot_launches(pkg, ctx, "k_primary")


@pytest.mark.parametrize("spp", SPPS)
def test_paths_across_batches(pkg, orc, ctx, golden, spp):
    """Recipe P (p11 at 240x135) with 1 to 4 batches: against the oracle, the counters, 3 shards; the launches of k_primary are
    those of one 16-sample batch times the number of batches."""
    scene = golden("p11_1080").scene(pkg)
    W, H = 240, 135
    cpu, cst = orc.render_paths(scene, W, H, spp, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=OT)
    fast = render_paths_gpu(pkg, ctx, scene, W, H, spp)
    check_paths(fast, cpu, orc, "p11 240x135 %d spp" % spp)
    frs = pkg.frame_setup(scene.desc.camera, W, H, samples=spp, gather_bounces=4, collect_stats=True)
    for attempt in range(3):  # (recipe P with counters reports a capacity overflow instead of repeating the batch; the report grew it)
        try:
            cnt, gst = ctx.render(frs, stats=True)
            break
        except pkg.RtuError as e:
            if e.code != pkg.RTU_ERR_CAPACITY or attempt == 2:
                raise
    assert np.array_equal(cnt.view(np.uint32), fast.view(np.uint32)), "fast and counting variants differ"
    assert gst == cst, "counters differ"
    three = render_paths_gpu(pkg, ctx, scene, W, H, spp, shard_count=3)
    assert np.array_equal(three.view(np.uint32), fast.view(np.uint32)), "3 shards differ from one"
    _, per_batch = _touched_primary_launches(pkg, ctx, scene, W, H, 16)
    img, total = _touched_primary_launches(pkg, ctx, scene, W, H, spp)
    assert np.array_equal(img.view(np.uint32), fast.view(np.uint32)), "touched-bytes frame differs"
    assert per_batch >= 1 and total == per_batch * math.ceil(spp / 16), (per_batch, total)


def _bands(H, n=8):
    return [(0, n), (H // 2 - n // 2, n), (H - n, n)]


def test_batches_shorter_than_16(pkg, orc, ctx, golden):
    """2560x1440: 2^25 / pixels = 9 samples per launch sequence, 20 spp = 9 + 9 + 2. Row bands against the oracle."""
    scene = golden("p10_s4_160x120").scene(pkg)
    W, H, spp = 2560, 1440, 20
    assert (1 << 25) // (W * H) == 9
    gpu, _ = render_gpu(pkg, ctx, scene, W, H, spp)
    for row0, n in _bands(H):
        cpu, _ = orc.render_samples(scene, W, H, spp, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=OT, row0=row0, nrows=n)
        check(gpu[row0:row0 + n], cpu, orc, spp, "rows %d-%d" % (row0, row0 + n - 1))


def test_config5_at_64_samples(pkg, orc, ctx, golden):
    """BASELINE config 5 at 64 spp (p11 at 1920x1080, recipe P: four batches of 16): 24 rows in three bands against the oracle."""
    g = golden("p11_1080")
    scene = g.scene(pkg)
    W, H, spp = g.width, g.height, 64
    gpu = render_paths_gpu(pkg, ctx, scene, W, H, spp)
    for row0, n in _bands(H):
        cpu, _ = orc.render_paths(scene, W, H, spp, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=OT, row0=row0, nrows=n)
        check_paths(gpu[row0:row0 + n], cpu, orc, "config 5, 64 spp, rows %d-%d" % (row0, row0 + n - 1))


def test_accumulators_start_over(pkg, orc, ctx, golden):
    """A 64-spp frame, then a 17-spp frame of a smaller shape on the same context: the second equals the frame rendered on a
    fresh context and the oracle (nothing of the first frame's sums or hit counts is carried over)."""
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    render_gpu(pkg, ctx, scene, g.width, g.height, 64)
    W, H, spp = 120, 90, 17
    after, _ = render_gpu(pkg, ctx, scene, W, H, spp)
    fresh_ctx = pkg.Context(0)
    try:
        fresh, _ = render_gpu(pkg, fresh_ctx, scene, W, H, spp)
    finally:
        fresh_ctx.close()
    assert np.array_equal(after.view(np.uint32), fresh.view(np.uint32)), "the earlier frame changes the later one"
    cpu, _ = orc.render_samples(scene, W, H, spp, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=OT)
    check(after, cpu, orc, spp, "17 spp after 64")


GLASSROOM = """<xml><scene>
  <object type="sphere" name="room" material="wall"><scale value="60"/></object>
  <object type="sphere" name="ball" material="glassmirror"><scale value="9"/><translate x="0" y="0" z="0"/></object>
  <material type="blinn" name="wall"><diffuse r="0.7" g="0.6" b="0.5"/><specular value="0.2"/><glossiness value="10"/></material>
  <material type="blinn" name="glassmirror"><diffuse r="0.1" g="0.1" b="0.1"/><specular value="0.8"/><glossiness value="60"/>
    <reflection value="0.4"/><refraction index="1.4" value="0.7"/></material>
  <light type="ambient" name="a"><intensity value="0.3"/></light>
  <light type="point" name="p"><intensity value="0.8"/><position x="10" y="-20" z="25"/></light>
</scene><camera><position x="0" y="-14" z="0"/><target x="0" y="0" z="0"/><up x="0" y="0" z="1"/><fov value="70"/>
  <width value="128"/><height value="96"/></camera></xml>"""


def test_capacity_retry_with_counters(pkg, orc, tmp_path):
    """The glass room of test_frame_capacity_overflow_is_detected_and_repaired (up to three child frames per pixel) in recipe S,
    40 spp, counters on, on a fresh context: its first batch runs out of frame records, render_sampled grows them and starts the
    frame again from sample 0 with the counters zeroed. Image and counters equal the oracle's."""
    xml = tmp_path / "glassroom.xml"
    xml.write_text(GLASSROOM)
    scene = pkg.Scene.from_xml(str(xml))
    W, H, spp = 128, 96, 40
    cpu, cst = orc.render_samples(scene, W, H, spp, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=OT)
    c = pkg.Context(0)
    try:
        img, gst = render_gpu(pkg, c, scene, W, H, spp, stats=True)
        check(img, cpu, orc, spp, "glass room")
        assert gst == cst, "counters differ"
        fast, _ = render_gpu(pkg, c, scene, W, H, spp)
        assert np.array_equal(fast.view(np.uint32), img.view(np.uint32)), "fast and counting variants differ"
    finally:
        c.close()
