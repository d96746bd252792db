"""Path-traced ray batches (rtu_shade_rays_paths / _device, include/rtu_render.h) against the recipe-P renders and the oracle.

As for the sampled batches, the oracle is reached through cameras: the rays and keys of sample k of a frame
(rtu_camera_sample_rays), shaded with eye = the camera, must be that sample's image of the frame with gather_bounces = 4 —
rtu_debug_sample_images — bit for bit (t at every ray, rgb at every hit ray), and meet the oracle's image of that sample
(rtu_oracle_render_sample_images with gi = 1) under the bar of tests/test_gpu_shade_rays_sampled.py: float z bit-exact, 8-bit RGB
within 1, linear RGB within 2e-4. Everything else is byte identity with what this established, plus rtu_trace_rays for t.
Rays no camera fires, and the gathered light itself, meet the oracle's keyed ray-level entry in tests/test_gpu_rays_keyed.py."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_ray_query import BIG, bits, set_camera
from test_gpu_shade_rays_sampled import against_oracle, check, environment_of, eye_of, families, same_bytes, scrambled
from test_mesh_update_host import clone

pytestmark = pytest.mark.gpu

TAGS = ["p11_p2_120x68", "p13_p2_96x72", "p10_s4_160x120", "teapot1_s2_160x90", "p9_s3_160x120", "teapot2_240x135"]
SPP = {"p10_s4_160x120": 3}  # 2 otherwise


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def sample_set(pkg, ctx, scene, W, H, spp, max_bounce=5):
    """The recipe-P frame, and per sample its rays, keys and the fast variant's shade of them. Uploads the scene."""
    ctx.upload(scene)
    frame = pkg.frame_setup(scene.desc.camera, W, H, samples=spp, max_bounce=max_bounce, gather_bounces=4)
    rays, keys, outs = [], [], []
    for k in range(spp):
        r, q = pkg.camera_sample_rays(frame, k)
        o = ctx.shade_rays_paths(r, q, eye_of(frame), max_bounce=max_bounce)[0]
        for a in (r, q, o):
            a.setflags(write=False)
        rays.append(r)
        keys.append(q)
        outs.append(o)
    return SimpleNamespace(scene=scene, W=W, H=H, spp=spp, frame=frame, eye=eye_of(frame), rays=rays, keys=keys, outs=outs)


@pytest.fixture(scope="module")
def cam(pkg, golden, ctx):
    """Per golden tag, computed once and left unchanged. The shared context holds some other scene afterwards."""
    cache = {}

    def get(tag):
        if tag not in cache:
            g = golden(tag)
            cache[tag] = sample_set(pkg, ctx, g.scene(pkg), g.width, g.height, SPP.get(tag, 2))
        return cache[tag]
    return get


def equals_the_render_and_the_oracle(pkg, orc, ctx, c, what, max_bounce=5, check=check):
    """Item 1 of the contract for one sample set (the scene is uploaded): (hit rays per sample, pixels whose samples all hit). check: the
    colour bar against the oracle (against_oracle of tests/test_gpu_shade_rays_sampled.py)."""
    hits = []
    acc = np.zeros((c.W * c.H, 3), np.float32)
    all_hit = np.ones(c.W * c.H, bool)
    for k in range(c.spp):
        out = c.outs[k]
        render = ctx.sample_images(c.frame, k, 1)[0].reshape(-1, 4)
        cpu = orc.sample_images(c.scene, c.W, c.H, c.spp, k, 1, gi=True, threads=8, max_bounce=max_bounce)[0]
        hit = out[:, 3] < BIG
        tbad = int((bits(out[:, 3]) != bits(render[:, 3])).sum())
        rbad = int((bits(out[hit, :3]) != bits(render[hit, :3])).any(axis=1).sum())
        obad = int((bits(out[:, 3]) != bits(cpu[..., 3].reshape(-1))).sum())
        d = np.abs(out[hit, :3].astype(np.float64) - cpu.reshape(-1, 4)[hit, :3].astype(np.float64))
        print("%s sample %d: %d rays, %d hit; t differs from the render's at %d, from the oracle's at %d; rgb from the render's at %d hit rays; "
              "largest linear difference from the oracle %.3g" % (what, k, len(out), int(hit.sum()), tbad, obad, rbad, d.max() if d.size else 0.0))
        assert tbad == 0 and rbad == 0 and obad == 0
        assert np.array_equal(against_oracle(out, cpu, orc, c.spp, "%s sample %d" % (what, k), check=check), hit)
        miss = ~hit
        if miss.any():
            assert same_bytes(out[miss, :3], environment_of(pkg, ctx, c.scene, c.rays[k]["dir"][miss]))
            assert np.array_equal(bits(out[miss, 3]), bits(c.rays[k]["tmax"][miss]))
        acc = acc + out[:, :3]
        all_hit &= hit
        hits.append(int(hit.sum()))
    mean = acc / np.float32(c.spp)
    frame_img = ctx.render(c.frame)[0].reshape(-1, 4)
    mbad = int((bits(mean[all_hit]) != bits(frame_img[all_hit, :3])).any(axis=1).sum())
    print("%s: the mean of the %d shades differs from the frame at %d of %d pixels whose samples all hit" % (what, c.spp, mbad, int(all_hit.sum())))
    assert mbad == 0
    return hits, int(all_hit.sum())


# ---- 1. camera-sample rays are the render's samples ------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_camera_sample_rays_are_the_renders_samples(pkg, orc, ctx, cam, tag):
    c = cam(tag)
    ctx.upload(c.scene)
    hits, all_hit = equals_the_render_and_the_oracle(pkg, orc, ctx, c, tag)
    assert min(hits) >= 300 and all_hit > 200, (hits, all_hit)  # (teapot1 at 160 x 90, spp 2: 309 and 308 of its rays hit, 282 pixels)
    if tag == "teapot1_s2_160x90":
        assert hits == [309, 308] and all_hit == 282  # the primary rays and keys are recipe S's
    if tag == "p11_p2_120x68":
        assert hits == [c.W * c.H] * c.spp  # every ray hits


# ---- 2. the gather is really there -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["p11_p2_120x68", "p10_s4_160x120"])
def test_the_gather_is_really_there(pkg, ctx, cam, tag):
    c = cam(tag)
    ctx.upload(c.scene)
    rays, keys, out = c.rays[0], c.keys[0], c.outs[0]
    direct = ctx.shade_rays_sampled(rays, keys, c.eye)[0]
    assert np.array_equal(bits(direct[:, 3]), bits(out[:, 3])), "t differs from recipe S's"
    hit = out[:, 3] < BIG
    differ = int((bits(direct[hit, :3]) != bits(out[hit, :3])).any(axis=1).sum())
    print("%s: %d of %d hit rays differ from direct lighting only" % (tag, differ, int(hit.sum())))
    assert differ > hit.sum() / 2
    other = ctx.shade_rays_paths(rays[hit], keys[hit] ^ np.uint32(1), c.eye)[0]
    changed = int((bits(other[:, :3]) != bits(out[hit, :3])).any(axis=1).sum())
    print("%s: %d of %d hit rays change colour with key ^ 1" % (tag, changed, int(hit.sum())))
    assert changed > 0 and np.array_equal(bits(other[:, 3]), bits(out[hit, 3]))


# ---- 3. the counting variant -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["p11_p2_120x68", "p10_s4_160x120", "teapot1_s2_160x90"])
def test_counting_variant(pkg, orc, ctx, cam, tag):
    c = cam(tag)
    ctx.upload(c.scene)
    _, cstats = orc.render_paths(c.scene, c.W, c.H, c.spp, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=8)
    total = None
    for k in range(c.spp):
        ref = ctx.shade_rays_paths(c.rays[k], c.keys[k], c.eye, reference_walk=True)[0]
        assert same_bytes(ref, c.outs[k]), "the counting variant's output differs from the fast variant's (sample %d)" % k
        ref2, st = ctx.shade_rays_paths(c.rays[k], c.keys[k], c.eye, stats=True)
        assert same_bytes(ref2, c.outs[k])
        total = st if total is None else {n: total[n] + st[n] for n in st}
    assert total == cstats, "counters of the %d batches differ from the oracle's of the frame: %s vs %s" % (c.spp, total, cstats)


# ---- 4. depths -------------------------------------------------------------------------------------------------------------------
def test_depths(pkg, orc, ctx, golden):
    g = golden("p13_p2_96x72")
    scene = g.scene(pkg)
    images = {}
    for mb in (0, 2, 5):
        c = sample_set(pkg, ctx, scene, g.width, g.height, 2, max_bounce=mb)
        equals_the_render_and_the_oracle(pkg, orc, ctx, c, "p13 max_bounce %d" % mb, max_bounce=mb)
        images[mb] = c.outs[0]
    assert not same_bytes(images[0], images[2])  # the depth does reach the recursion (Project13 has glass and mirrors)


# ---- 5. lens ---------------------------------------------------------------------------------------------------------------------
def test_depth_of_field(pkg, orc, ctx, golden):
    g = golden("p10_s4_160x120")
    scene = clone(pkg, g.scene(pkg))
    scene.desc.camera.dof = 0.4
    scene.desc.camera.focaldist = 20.0
    c = sample_set(pkg, ctx, scene, g.width, g.height, 2)
    assert c.frame.dof > 0
    for k in range(c.spp):
        assert len(np.unique(c.rays[k]["org"], axis=0)) > 0.9 * c.rays[k].size  # every ray has its own origin
    hits, all_hit = equals_the_render_and_the_oracle(pkg, orc, ctx, c, "p10 with a lens")
    assert min(hits) >= 300 and all_hit > 200


# ---- 6. other origins, with the oracle -------------------------------------------------------------------------------------------
def other_cameras(c, tag):
    """Four look-at cameras (set_camera of tests/test_gpu_ray_query.py): drawn around the golden's camera and around the middle of
    what it sees, aimed into what it sees."""
    out0 = c.outs[0]
    hit = out0[:, 3] < BIG
    p = c.rays[0]["org"][hit].astype(np.float64) + c.rays[0]["dir"][hit].astype(np.float64) * out0[hit, 3:4].astype(np.float64)
    lo, hi = np.percentile(p, 10, axis=0), np.percentile(p, 90, axis=0)
    mid, ext = (lo + hi) / 2, np.maximum(hi - lo, 1.0)
    eye = np.array(c.eye, np.float64)
    rng = np.random.RandomState(20261019 + len(tag))
    cams = []
    for k in range(4):
        base = eye if k % 2 == 0 else (eye + mid) / 2
        pos = base + rng.uniform(-0.25, 0.25, 3) * ext
        target = mid + rng.uniform(-0.3, 0.3, 3) * ext
        cams.append((pos, target, float(rng.uniform(30, 90))))
    return cams


@pytest.mark.parametrize("tag", ["p10_s4_160x120", "p13_p2_96x72"])
def test_other_origins_against_the_oracle(pkg, orc, ctx, cam, tag):
    c = cam(tag)
    ctx.upload(c.scene)
    W, H, spp = 48, 36, 2
    hits = 0
    for j, (pos, target, fov) in enumerate(other_cameras(c, tag)):
        s = clone(pkg, c.scene)
        set_camera(s, pos, target, fov=fov)
        frame = pkg.frame_setup(s.desc.camera, W, H, samples=spp, gather_bounces=4)
        for k in range(spp):
            rays, keys = pkg.camera_sample_rays(frame, k)
            out = ctx.shade_rays_paths(rays, keys, eye_of(frame))[0]
            cpu = orc.sample_images(s, W, H, spp, k, 1, gi=True, threads=8)[0]
            assert np.array_equal(bits(out[:, 3]), bits(cpu[..., 3].reshape(-1))), "camera %d sample %d: t differs from the oracle's" % (j, k)
            hit = against_oracle(out, cpu, orc, spp, "%s camera %d sample %d" % (tag, j, k))
            assert np.array_equal(hit, out[:, 3] < BIG)
            hits += int(hit.sum())
    print("%s: %d hit rays from four other cameras" % (tag, hits))
    assert hits > 4 * spp * 300


# ---- 7. per-ray answers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["p10_s4_160x120", "p11_p2_120x68"])
def test_the_answer_is_the_rays_not_the_indexs(pkg, ctx, cam, tag):
    c = cam(tag)
    ctx.upload(c.scene)
    rays, keys, out = c.rays[1], c.keys[1], c.outs[1]
    assert same_bytes(ctx.shade_rays_paths(rays[::-1], keys[::-1], c.eye)[0], out[::-1]), "reversed"
    r, q, src = scrambled(rays, keys)
    valid = src >= 0
    assert (~valid).sum() >= 8 * 10 and r.size > rays.size * 8 // 7  # (an invalid ray of each of the eight kinds, at least ten times)
    want = np.zeros((r.size, 4), np.float32)
    want[valid] = out[src[valid]]
    for ref in (False, True):
        got = ctx.shade_rays_paths(r, q, c.eye, reference_walk=ref)[0]
        assert not got[~valid].view(np.uint8).any(), "an invalid ray must give sixteen zero bytes"
        bad = int((bits(got) != bits(want)).any(axis=1).sum())
        print("%s ref=%s: %d rays (%d invalid), %d differ from their ray's bytes" % (tag, ref, r.size, int((~valid).sum()), bad))
        assert bad == 0
    for n in (1, 63, 64, 65, 4097):
        assert (n < 200 or (src[300:300 + n] < 0).any())
        assert same_bytes(ctx.shade_rays_paths(r[300:300 + n], q[300:300 + n], c.eye)[0], want[300:300 + n]), n
        assert same_bytes(ctx.shade_rays_paths(r[:n], q[:n], c.eye)[0], want[:n]), n


# ---- 8. rays no camera fires -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["p10_s4_160x120", "p11gs_s2_160x90"])
def test_rays_no_camera_fires(pkg, ctx, cam, tag):
    c = cam(tag)
    ctx.upload(c.scene)
    hits = 0
    for name, rays in families(pkg, c):
        keys = np.array([pkg.sample_key(i, 7) for i in range(rays.size)], np.uint32)
        out = ctx.shade_rays_paths(rays, keys, c.eye)[0]
        q = ctx.trace_rays(rays)
        assert not (q["flags"] & pkg.RTU_RAY_INVALID).any()
        hit = (q["flags"] & pkg.RTU_RAY_HIT) != 0
        assert np.array_equal(bits(out[:, 3]), bits(q["t"])), name + ": t differs from rtu_trace_rays"
        assert np.array_equal(out[:, 3] < BIG, hit), name + ": the hit flag differs from rtu_trace_rays"
        assert same_bytes(ctx.shade_rays_paths(rays, keys, c.eye, reference_walk=True)[0], out), name + ": fast and reference walk differ"
        assert same_bytes(ctx.shade_rays_paths(rays, keys, c.eye)[0], out), name + ": two runs differ"
        if (~hit).any():
            assert same_bytes(out[~hit, :3], environment_of(pkg, ctx, c.scene, rays["dir"][~hit]))
        hits += int(hit.sum())
        print("%s %s: %d rays, %d hit" % (tag, name, rays.size, int(hit.sum())))
    assert hits > 1000


# ---- 9. switches -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["p13_p2_96x72", "teapot1_s2_160x90"])
def test_switches_change_no_byte(pkg, ctx, cam, tag):
    c = cam(tag)
    ctx.upload(c.scene)
    hip, h = pkg.hip, ctx._h
    rays, keys, out = c.rays[0], c.keys[0], c.outs[0]

    def shade():
        return ctx.shade_rays_paths(rays, keys, c.eye)[0]
    try:
        for flag in (64, 2048):
            assert hip.rtu_debug_flags(h, flag) == pkg.RTU_OK
            assert same_bytes(shade(), out), "rtu_debug_flags %d" % flag
        assert hip.rtu_debug_flags(h, 0) == pkg.RTU_OK
        for level in range(1, 7):
            assert hip.rtu_debug_tail_from(h, level) == pkg.RTU_OK
            assert same_bytes(shade(), out), "rtu_debug_tail_from %d" % level
            # the forced level did reach the shading steps (the chain steps, which launch() sees first, have no levels to cut)
            assert hip.rtu_debug_last_tail_from(h) == level
        spent = []
        for _ in range(2):  # ... and is spent: whatever cut level the next shades learn, it is the same twice, forced by nobody
            assert same_bytes(shade(), out)
            spent.append(hip.rtu_debug_last_tail_from(h))
        assert spent[0] == spent[1] and 1 <= spent[0] <= 6, spent
        assert hip.rtu_debug_tail_from(h, 1) == pkg.RTU_OK  # the counting variant has no tail, forced or not
        assert same_bytes(ctx.shade_rays_paths(rays, keys, c.eye, reference_walk=True)[0], out) and hip.rtu_debug_last_tail_from(h) == 6
        assert hip.rtu_debug_node_bounds(h, 0) == pkg.RTU_OK
        assert same_bytes(shade(), out), "rtu_debug_node_bounds(0)"
        ctx.upload(c.scene)  # (the two scene hooks last until the next upload)
        assert hip.rtu_debug_walk_stack_limit(h, 3) == pkg.RTU_OK
        assert same_bytes(shade(), out), "rtu_debug_walk_stack_limit(3)"
    finally:
        hip.rtu_debug_flags(h, 0)
        ctx.upload(c.scene)


# ---- 10. neighbours --------------------------------------------------------------------------------------------------------------
def test_renders_and_shades_leave_each_other_alone(pkg, cam, golden):
    c = cam("p11_p2_120x68")
    plain = golden("teapot2_240x135").scene(pkg)
    ctx = pkg.Context(0)
    try:
        ctx.upload(c.scene)
        before = ctx.render(c.frame)[0]
        assert same_bytes(ctx.shade_rays_paths(c.rays[0], c.keys[0], c.eye)[0], c.outs[0])
        assert same_bytes(ctx.render(c.frame)[0], before)
        # path batches, sampled batches, unsampled batches and frames in turn: nothing is allocated after the first round
        ctx.upload(plain)
        pf = pkg.frame_setup(plain.desc.camera, 96, 64)
        pr = pkg.camera_rays(pf)
        sf = pkg.frame_setup(plain.desc.camera, 96, 64, samples=2)
        gf = pkg.frame_setup(plain.desc.camera, 96, 64, samples=2, gather_bounces=4)
        sr, sk = pkg.camera_sample_rays(sf, 1)
        first, a1 = None, None
        for k in range(5):
            got = (ctx.shade_rays_paths(sr, sk, eye_of(sf))[0], ctx.shade_rays_sampled(sr, sk, eye_of(sf))[0], ctx.shade_rays(pr, eye_of(pf))[0],
                   ctx.render(pf)[0], ctx.render(sf)[0], ctx.render(gf)[0])
            if k == 0:
                first = got
            if k == 1:
                a1 = pkg.hip.rtu_debug_device_allocations()  # (they have alternated twice)
            assert all(same_bytes(x, y) for x, y in zip(got, first))
        assert pkg.hip.rtu_debug_device_allocations() == a1
    finally:
        ctx.close()


def test_an_open_progressive_session_is_not_disturbed(pkg, ctx, cam):
    c = cam("p10_s4_160x120")
    ctx.upload(c.scene)
    f = pkg.frame_setup(c.scene.desc.camera, 96, 72, samples=4, gather_bounces=4)
    p = ctx.progressive(f)
    try:
        p.advance(2)
        snap0, _ = p.snapshot()
        assert same_bytes(ctx.shade_rays_paths(c.rays[0], c.keys[0], c.eye)[0], c.outs[0])
        snap1, _ = p.snapshot()
        assert same_bytes(snap0, snap1)
        assert p.status()[0] == 2
        p.advance(2)
        assert same_bytes(p.snapshot()[0], ctx.render(f)[0])
    finally:
        p.close()


def test_shades_follow_scene_updates(pkg, cam):
    from test_gpu_ray_query import lights
    from test_light_lists import RtuLight
    c = cam("p10_s4_160x120")
    rays, keys = c.rays[0], c.keys[0]

    def fresh(scene):
        f = pkg.Context(0)
        try:
            f.upload(scene)
            return f.shade_rays_paths(rays, keys, c.eye)[0]
        finally:
            f.close()
    ctx = pkg.Context(0)
    try:
        ctx.upload(c.scene)
        assert same_bytes(ctx.shade_rays_paths(rays, keys, c.eye)[0], c.outs[0])
        hard = clone(pkg, c.scene)
        soft = [i for i in range(hard.desc.n_lights) if lights(hard)[i].size > 0]
        assert soft, "p10 has a soft light"
        for i in soft:  # a soft light made hard
            l = RtuLight.from_buffer_copy(bytes(lights(hard)[i]))
            l.size = 0.0
            hard.set_light(i, l)
        ctx.update(hard)
        out1 = ctx.shade_rays_paths(rays, keys, c.eye)[0]
        assert not same_bytes(out1, c.outs[0])
        assert same_bytes(out1, fresh(hard))
        ctx.update(c.scene)
        assert same_bytes(ctx.shade_rays_paths(rays, keys, c.eye)[0], c.outs[0])
    finally:
        ctx.close()


def device_buffers(rays, keys, fill=0.0):
    import torch
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).to("cuda:0")
    d_keys = torch.from_numpy(np.ascontiguousarray(keys).view(np.int32).copy()).to("cuda:0")
    d_out = torch.full((rays.size * 4,), fill, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    return d_rays, d_keys, d_out


def test_the_device_form_on_a_callers_stream_equals_the_host_form(pkg, ctx, cam):
    import torch
    c = cam("p13_p2_96x72")
    ctx.upload(c.scene)
    rays, keys, out = c.rays[1], c.keys[1], c.outs[1]
    stream = torch.cuda.Stream(device=0)
    d_rays, d_keys, d_out = device_buffers(rays, keys, 7.0)
    for ref in (False, True):
        for attempt in range(8):
            ctx.shade_rays_paths_device(d_rays.data_ptr(), d_keys.data_ptr(), rays.size, c.eye, d_out.data_ptr(), stream.cuda_stream, reference_walk=ref)
            try:
                ctx.frame_status()
                break
            except pkg.RtuError as err:
                assert err.code == pkg.RTU_ERR_CAPACITY
        else:
            raise AssertionError("capacity never sufficed")
        assert same_bytes(d_out.cpu().numpy().reshape(-1, 4), out)
        d_out.fill_(7.0)
        torch.cuda.synchronize()


# ---- 11. capacity ----------------------------------------------------------------------------------------------------------------
GLOSSROOM = """<xml><scene>
  <object type="sphere" name="room" material="wall"><scale value="60"/></object>
  <object type="sphere" name="ball" material="glassmirror"><scale value="9"/><translate x="0" y="0" z="0"/></object>
  <material type="blinn" name="wall"><diffuse r="0.7" g="0.6" b="0.5"/><specular value="0.2"/><glossiness value="10"/></material>
  <material type="blinn" name="glassmirror"><diffuse r="0.1" g="0.1" b="0.1"/><specular value="0.8"/><glossiness value="60"/>
    <reflection value="0.4" glossiness="0.05"/><refraction index="1.4" value="0.7" glossiness="0.03"/></material>
  <light type="ambient" name="a"><intensity value="0.3"/></light>
  <light type="point" name="p"><intensity value="0.8"/><position x="10" y="-20" z="25"/><size value="2"/></light>
</scene><camera><position x="0" y="-14" z="0"/><target x="0" y="0" z="0"/><up x="0" y="0" z="1"/><fov value="70"/>
  <width value="128"/><height value="96"/></camera></xml>"""


def test_capacity_overflow_is_reported_and_repaired(pkg, orc, tmp_path):
    """A glossy glass-and-mirror ball in a room under a soft light: up to three child frames per Shade() call, two Shade() trees per
    chain hit, and a fresh context provisions one frame per level-0 frame."""
    xml = tmp_path / "glossroom.xml"
    xml.write_text(GLOSSROOM)
    scene = pkg.Scene.from_xml(str(xml))
    W, H = 128, 96
    frame = pkg.frame_setup(scene.desc.camera, W, H, samples=1, gather_bounces=4)
    rays, keys = pkg.camera_sample_rays(frame, 0)
    cpu = orc.sample_images(scene, W, H, 1, 0, 1, gi=True, threads=8)[0]
    c = pkg.Context(0)  # a fresh context: nothing learned, nothing grown
    try:
        c.upload(scene)
        d_rays, d_keys, d_out = device_buffers(rays, keys)

        def shade():
            c.shade_rays_paths_device(d_rays.data_ptr(), d_keys.data_ptr(), rays.size, eye_of(frame), d_out.data_ptr())
        shade()
        with pytest.raises(pkg.RtuError) as e:
            c.frame_status()
        assert e.value.code == pkg.RTU_ERR_CAPACITY  # it did overflow: otherwise nothing is tested
        for attempt in range(8):  # every report grows the capacity of at least one more recursion level
            shade()
            try:
                c.frame_status()
                break
            except pkg.RtuError as err:
                assert err.code == pkg.RTU_ERR_CAPACITY
        else:
            raise AssertionError("capacity never sufficed")
        print("the device form succeeded at repeat %d" % (attempt + 1))
        dev = d_out.cpu().numpy().reshape(-1, 4)
        assert against_oracle(dev, cpu, orc, 1, "glossroom").sum() > 1000
    finally:
        c.close()
    c2 = pkg.Context(0)  # the host form on another fresh context: repairs itself
    try:
        c2.upload(scene)
        host = c2.shade_rays_paths(rays, keys, eye_of(frame))[0]
        c2.frame_status()
        assert same_bytes(host, dev)
    finally:
        c2.close()


# ---- 12. errors ------------------------------------------------------------------------------------------------------------------
def test_errors(pkg, cam):
    c = cam("p10_s4_160x120")
    hip = pkg.hip
    r = np.ascontiguousarray(c.rays[0][:8])
    q = np.ascontiguousarray(c.keys[0][:8])
    q_off = np.zeros(40, np.uint8)  # (a key buffer that is not 4-byte aligned)
    out = np.zeros((8, 4), np.float32)
    ctx = pkg.Context(0)
    try:
        h = ctx._h
        ok = pkg.shade_desc(c.eye)

        def host(desc, rays=r.ctypes.data, keys=q.ctypes.data, o=out.ctypes.data, n=8):
            rc = hip.rtu_shade_rays_paths(h, rays, keys, n, ctypes.byref(desc) if desc is not None else None, o, None)
            ctx.frame_status()  # clean afterwards
            return rc

        def device(desc, rays=4096, keys=16384, o=8192, n=8):  # (every case below is refused before a pointer is read)
            rc = hip.rtu_shade_rays_paths_device(h, rays, keys, n, ctypes.byref(desc) if desc is not None else None, o, None)
            ctx.frame_status()
            return rc
        assert host(ok) == pkg.RTU_ERR_NO_SCENE and device(ok) == pkg.RTU_ERR_NO_SCENE
        ctx.upload(c.scene)
        assert host(ok) == pkg.RTU_OK
        assert same_bytes(out, c.outs[0][:8])
        # the unsampled call still refuses the scene
        assert hip.rtu_shade_rays(h, r.ctypes.data, 8, ctypes.byref(ok), out.ctypes.data, None) == pkg.RTU_ERR_STOCHASTIC
        assert hip.rtu_shade_rays_device(h, 4096, 8, ctypes.byref(ok), 8192, None) == pkg.RTU_ERR_STOCHASTIC
        ctx.frame_status()
        # n == 0: fine, whatever the pointers, and nothing is launched
        counts = ctx.frame_counts()
        assert host(ok, None, None, None, 0) == pkg.RTU_OK and device(ok, None, None, None, 0) == pkg.RTU_OK
        assert ctx.frame_counts() == counts
        assert ctx.shade_rays_paths(c.rays[0][:0], c.keys[0][:0], c.eye)[0].shape == (0, 4)
        # NULL pointers with n > 0
        assert host(ok, None) == pkg.RTU_ERR_ARG and host(ok, o=None) == pkg.RTU_ERR_ARG and host(None) == pkg.RTU_ERR_ARG
        assert device(ok, None) == pkg.RTU_ERR_ARG and device(ok, o=None) == pkg.RTU_ERR_ARG and device(None) == pkg.RTU_ERR_ARG
        assert host(ok, keys=None) == pkg.RTU_ERR_ARG and device(ok, keys=None) == pkg.RTU_ERR_ARG
        # keys that are not 4-byte aligned; device pointers that are not 16-byte aligned
        base = q_off.ctypes.data + (-q_off.ctypes.data) % 4
        for off in (1, 2, 3):
            assert host(ok, keys=base + off) == pkg.RTU_ERR_ARG and device(ok, keys=16384 + off) == pkg.RTU_ERR_ARG
        assert device(ok, rays=4096 + 8) == pkg.RTU_ERR_ARG and device(ok, o=8192 + 4) == pkg.RTU_ERR_ARG
        # more chains than a launch sequence of recipe P takes, in the device form
        assert device(ok, n=(1 << 25) + 1) == pkg.RTU_ERR_ARG
        for flags in (2, 4, 0x80000000, 3):
            d = pkg.shade_desc(c.eye)
            d.flags = flags
            assert host(d) == pkg.RTU_ERR_ARG and device(d) == pkg.RTU_ERR_ARG
        for k in range(3):
            d = pkg.shade_desc(c.eye)
            d.reserved[k] = 1
            assert host(d) == pkg.RTU_ERR_ARG and device(d) == pkg.RTU_ERR_ARG
        for mb in (-1, 6, 1 << 30):
            d = pkg.shade_desc(c.eye)
            d.max_bounce = mb
            assert host(d) == pkg.RTU_ERR_ARG and device(d) == pkg.RTU_ERR_ARG
        for k, v in ((0, float("nan")), (1, float("inf")), (2, float("-inf"))):
            d = pkg.shade_desc(c.eye)
            d.eye[k] = v
            assert host(d) == pkg.RTU_ERR_ARG and device(d) == pkg.RTU_ERR_ARG
        assert hip.rtu_shade_rays_paths(None, r.ctypes.data, q.ctypes.data, 8, ctypes.byref(ok), out.ctypes.data, None) == pkg.RTU_ERR_ARG
        with pytest.raises(pkg.RtuError):
            ctx.shade_rays_paths_device(None, None, 8, c.eye, None)
        # RtuRay.reserved stays ignored
        r2 = r.copy()
        r2["reserved"] = 0xDEADBEEF
        assert host(ok, rays=r2.ctypes.data) == pkg.RTU_OK and same_bytes(out, c.outs[0][:8])
        # the context still works
        assert host(ok) == pkg.RTU_OK and same_bytes(out, c.outs[0][:8])
    finally:
        ctx.close()
