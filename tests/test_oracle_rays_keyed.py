"""The oracle's keyed ray-level entry (rtu_oracle_rays_keyed: oracle_binding.shade_rays_sampled / shade_rays_paths / gather_rays /
shade_rays_ambient) against the oracle's own sampled renders, and the ray families of tests/test_gpu_rays_keyed.py with the properties
that make them worth shading. No GPU.

The camera path of the oracle is the part validated against the live reference build (tests/test_oracle.py), so the entry is tied to
it bit for bit: fed the rays and keys of sample k of a recipe S / P frame it must give that sample's image (sample_images), all 16
bytes at every hit ray. Then the identities between the four modes, independence of order / batch / thread count, the counters,
the refusals, and the bytes of the unkeyed entry rtu_oracle_rays, pinned by hash from before the keyed entry was added.

The families (K1 probes, K2 surface starts, K3 keys, K4 sensors, K5 random scenes) are rays no camera fires; what each must contain to
test anything is asserted here on the oracle alone: root hits on back faces, gather chains that reach depth 4 and chains that leave
the scene at each of the depths 1 to 4, partial soft shadows, glossy roots, misses. The thresholds of the irradiance-map comparison
of tests/test_gpu_irradiance.py are chosen here as well, on the oracle's own chain, with their margin."""
import hashlib
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import PATH_TAGS
from test_fuzz_host import FAMILY_SIZE, S_SEEDS, ray_families, s_scene
from test_gpu_ray_query import bits, lights, materials
from test_irradiance_host import neighbours, pass_points
from test_light_lists import RtuLight
from test_mesh_update_host import clone
from test_oracle_rays import BIG, family_b, make_rays, probe_dirs, renormalised, valid
from test_sensor_host import camera_basis

F = np.float32
KEYED_TAGS = ["p10_s4_160x120", "p11x86_s1_120x90", "p11g_s2_160x90", "p11_p2_120x68", "p13_p2_96x72"]
SOFT_TAGS = ["p10_s4_160x120", "p11x86_s1_120x90"]                         # point lights with a size
GLOSSY_TAGS = ["p10_s4_160x120", "p11x86_s1_120x90", "p11g_s2_160x90"]     # glossy reflection / refraction
OPEN_TAGS = ["p10_s4_160x120", "p11g_s2_160x90", "p11_p2_120x68", "p13_p2_96x72"]  # rays can leave the scene (p11x86 is a closed room)
MAX_BATCH = 4096
THREADS = 8


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def sample_keys(pkg, n, sample):
    return np.array([pkg.sample_key(i, sample) for i in range(n)], np.uint32)


def plain_copy(pkg, scene):
    """The scene without its stochastic features (no lens, no light size, no glossiness): the same geometry, which the unkeyed entry
    rtu_oracle_rays accepts — for the closest hits (p, N) that the surface families start from."""
    out = clone(pkg, scene)
    out.desc.camera.dof = 0.0
    for i in range(out.desc.n_lights):
        if lights(out)[i].size > 0:
            l = RtuLight.from_buffer_copy(bytes(lights(out)[i]))
            l.size = 0.0
            out.set_light(i, l)
    for i in range(out.desc.n_materials):
        m = materials(out)[i]
        m.reflection_glossiness = 0.0
        m.refraction_glossiness = 0.0
    return out


def eye_of(scene):
    return tuple(float(x) for x in scene.desc.camera.pos)


def environment(orc, scene, dirs):
    """environment.SampleEnvironment(dir) from the oracle's texture arithmetic (as tests/test_oracle_rays.py does for a miss)."""
    d = scene.desc
    colour = np.array(list(d.environment.color), F)
    dirs = np.ascontiguousarray(dirs, F)
    if d.environment.has_map and not d.environment.map_is_null and d.environment_map.present:
        uvw = orc.texcoords(orc.TEXOP_ENV_UVW, dirs)
        return np.ascontiguousarray(colour[None, :] * orc.texcoords(orc.TEXOP_MAP, uvw, -2, scene), F)
    if d.environment.has_map:
        return np.ascontiguousarray(np.broadcast_to(colour * F(0), dirs.shape), F)
    return np.ascontiguousarray(np.broadcast_to(colour, dirs.shape), F)


# ---- the families ----------------------------------------------------------------------------------------------------------------
def probe_points(pkg, scene):
    """Two points inside the scene: a fifth and three fifths of the way from the middle of its box to the camera."""
    box = pkg.scene_sort_box(scene).astype(np.float64)
    centre, pos = 0.5 * (box[:3] + box[3:]), np.array(eye_of(scene))
    return [tuple(float(F(x)) for x in centre + f * (pos - centre)) for f in (0.2, 0.6)]


def family_k1(pkg, scene):
    """K1 probes: the 64 x 33 equirectangular directions of tests/test_oracle_rays.py (exact poles, an exact equator) from the two
    probe points, keys sample_key(i, 3 + probe). -> [(name, rays, keys)]"""
    d = probe_dirs()
    return [("probe %s" % (o,), make_rays(pkg, np.broadcast_to(np.array(o, F), d.shape), d), sample_keys(pkg, len(d), 3 + j))
            for j, o in enumerate(probe_points(pkg, scene))]


def family_k2(pkg, orc, scene):
    """K2 surface starts: from every second hit point of the first probe along N, -N and the mirror direction (family_d of
    tests/test_oracle_rays.py), keys sample_key(i, 5). The -N rays start on the inner side of whatever the probe saw."""
    probe = family_k1(pkg, scene)[0][1]
    h = orc.trace_rays(plain_copy(pkg, scene), probe, threads=THREADS)
    hit = np.flatnonzero((h["flags"] & orc.RAY_HIT) != 0)[::2]
    p, N, d = h["p"][hit], h["N"][hit], probe["dir"][hit]
    k = F(2) * ((d[:, 0] * N[:, 0] + d[:, 1] * N[:, 1]) + d[:, 2] * N[:, 2])
    rays = np.concatenate([make_rays(pkg, p, N), make_rays(pkg, p, -N), make_rays(pkg, p, renormalised(d - N * k[:, None]))])
    rays = rays[valid(rays)]  # (a hit with a NaN normal cannot start a valid ray)
    assert 900 < rays.size <= MAX_BATCH
    return [("surface starts", rays, sample_keys(pkg, rays.size, 5))]


def k3_keys(pkg):
    """64 keys: the corners of the 32-bit range, child keys of them, twenty sample keys, and the first 24 again at other indices."""
    keys = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
    keys += [pkg.child_key(k, s) for k in (0, 0x80000000, 0xFFFFFFFF) for s in range(5)]
    keys += [pkg.sample_key(977 * i, i) for i in range(20)]
    keys += keys[:24]
    assert len(keys) == 64 and len(set(keys)) == 40 and sum(k >= 1 << 31 for k in set(keys)) >= 8
    return np.array(keys, np.uint32)


def partial_shadow(orc, scene, rays, keys):
    """(shadow rays towards lights with a size, those of them that are occluded) per ray, summed over four keys: the ray's and three
    derived ones."""
    fired, occluded = np.zeros(rays.size, np.int64), np.zeros(rays.size, np.int64)
    for j in range(4):
        info = orc.keyed_info(scene, rays, keys ^ np.uint32(0x9E3779B9 * j & 0xFFFFFFFF), threads=THREADS)
        fired, occluded = fired + info[:, 2], occluded + info[:, 3]
    return fired, occluded


def family_k3(pkg, orc, scene):
    """K3 keys: one ray of the first probe, 64 times under k3_keys() — the middle one of those whose root hit is a lit front face and,
    where the scene has lights with a size, lies in a penumbra."""
    _, rays, keys = family_k1(pkg, scene)[0]
    f = orc.keyed_info(scene, rays, keys, threads=THREADS)[:, 0]
    want = orc.INFO_HIT | orc.INFO_FRONT | orc.INFO_MATERIAL
    fired, occluded = partial_shadow(orc, scene, rays, keys)
    ok = (f & want) == want
    if (ok & (fired > 0)).any():
        ok &= (occluded > 0) & (occluded < fired)
    idx = np.flatnonzero(ok)
    one = rays[idx[len(idx) // 2]]
    return [("one ray, 64 keys", np.repeat(one, 64), k3_keys(pkg))]


SENSOR_W, SENSOR_H, SENSOR_SAMPLES = 48, 24, 3
SENSOR_TAGS = {"p10_s4_160x120": 0, "p13_p2_96x72": 4}  # tag -> gather_bounces


def k4_sensors(pkg, scene, gather_bounces):
    """K4 sensors at the first probe point, in the camera's frame, 48 x 24 with 3 samples: a 200-degree fisheye, an equirectangular
    panorama and an orthographic window of 40 x 20 units."""
    _, right, up, fwd = camera_basis(scene)
    pos = probe_points(pkg, scene)[0]
    return [(model, pkg.sensor_desc(model, SENSOR_W, SENSOR_H, pos, right, up, fwd, samples=SENSOR_SAMPLES, gather_bounces=gather_bounces,
                                    fov_deg=200.0, extent=(40.0, 20.0))) for model in ("fisheye", "equirect", "ortho")]


def family_k5(pkg, orc, scene, seed):
    """K5: the families R1-R4 of tests/test_fuzz_host.py on a stochastic random scene, each cut to its first 2048 rays; keys
    sample_key(i, family)."""
    plain = plain_copy(pkg, scene)
    fam = ray_families(pkg, orc, scene, seed, trace=lambda r: orc.trace_rays(plain, r, threads=THREADS))
    return [(name, np.ascontiguousarray(rays[:FAMILY_SIZE]), sample_keys(pkg, min(rays.size, FAMILY_SIZE), j)) for j, (name, rays) in enumerate(fam)]


def contents(orc, scene, rays, keys):
    """What a batch holds, from rtu_oracle_rays_keyed_info: counts by name. partial: the rays of which, over four keys (the batch's and
    three derived ones), at least one but not all shadow rays towards lights with a size are occluded."""
    info = orc.keyed_info(scene, rays, keys, threads=THREADS)
    f = info[:, 0]
    hit, lit = (f & orc.INFO_HIT) != 0, (f & orc.INFO_MATERIAL) != 0
    fired, occluded = partial_shadow(orc, scene, rays, keys)
    out = dict(rays=rays.size, hits=int(hit.sum()), misses=int((~hit).sum()), back=int((hit & ((f & orc.INFO_FRONT) == 0)).sum()),
               glossy=int(((f & orc.INFO_GLOSSY) != 0).sum()), partial=int(((occluded > 0) & (occluded < fired)).sum()))
    for d in range(1, 5):
        out["leaves%d" % d] = int((lit & (info[:, 1] == d - 1)).sum())
    out["depth4"] = int((lit & (info[:, 1] == 4)).sum())
    return out


@pytest.fixture(scope="module")
def scenes(pkg, golden):
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = golden(tag).scene(pkg)
        return cache[tag]
    return get


# ==== the entry against the sampled renders =======================================================================================
@pytest.mark.parametrize("max_bounce", [5, 1])
@pytest.mark.parametrize("tag", ["p10_s4_160x120", "p9_s3_160x120"] + PATH_TAGS)
def test_camera_sample_rays_reproduce_the_sample_images(pkg, orc, golden, scenes, tag, max_bounce):
    g, scene = golden(tag), scenes(tag)
    W, H, spp = g.width, g.height, 2
    if tag == "p9_s3_160x120":
        assert scene.desc.camera.dof > 0  # depth of field: every ray has its own origin
    frame = pkg.frame_setup(scene.desc.camera, W, H, samples=spp, max_bounce=max_bounce)
    eye = tuple(frame.cam_pos)
    for gi, entry in ((False, orc.shade_rays_sampled), (True, orc.shade_rays_paths)):
        for k in range(spp):
            rays, keys = pkg.camera_sample_rays(frame, k)
            assert valid(rays).all()
            img = orc.sample_images(scene, W, H, spp, k, 1, gi=gi, threads=THREADS, max_bounce=max_bounce)[0].reshape(-1, 4)
            out = entry(scene, rays, keys, eye, max_bounce=max_bounce, threads=THREADS)[0]
            hit = img[:, 3] != BIG
            assert hit.sum() > 1000
            assert np.array_equal(bits(out[hit]), bits(img[hit])), "%s gi=%s sample %d: a hit ray differs from the sample image" % (tag, gi, k)
            assert np.array_equal(bits(out[:, 3]), bits(img[:, 3])), "t differs"  # (a miss: tmax = RTU_BIGFLOAT, the image's z)
            if (~hit).any():
                assert same_bytes(out[~hit, :3], environment(orc, scene, rays["dir"][~hit]))
    assert orc.max_bounce_now() == orc.MAX_BOUNCE


def test_a_miss_is_the_environment_and_tmax(pkg, orc, scenes):
    scene = scenes("p10_s4_160x120")
    assert scene.desc.environment.has_map
    _, rays, keys = family_k1(pkg, scene)[1]
    rays = rays.copy()
    rays["tmax"] = F(30.0)
    s = orc.shade_rays_sampled(scene, rays, keys, eye_of(scene), threads=THREADS)[0]
    miss = s[:, 3] == F(30.0)
    info = orc.keyed_info(scene, rays, keys, threads=THREADS)
    assert np.array_equal(miss, (info[:, 0] & orc.INFO_HIT) == 0) and miss.sum() > 500 and (~miss).sum() > 20
    env = environment(orc, scene, rays["dir"][miss])
    assert len(np.unique(env, axis=0)) > 50  # a picture, not a constant
    zero = np.zeros((rays.size, 4), F)
    for out in (s, orc.shade_rays_paths(scene, rays, keys, eye_of(scene), threads=THREADS)[0],
                orc.shade_rays_ambient(scene, rays, keys, zero, eye_of(scene), threads=THREADS)[0]):
        assert same_bytes(out[miss, :3], env) and np.all(out[miss, 3] == F(30.0))
    g = orc.gather_rays(scene, rays, keys, eye_of(scene), threads=THREADS)[0]
    assert not g[miss, :3].view(np.uint32).any() and np.all(g[miss, 3] == F(30.0))
    assert same_bytes(g[:, 3], s[:, 3])


# ---- identities ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", KEYED_TAGS)
def test_ambient_of_gather_is_paths(pkg, orc, scenes, tag):
    scene, eye = scenes(tag), eye_of(scenes(tag))
    for name, rays, keys in family_k1(pkg, scene) + family_k2(pkg, orc, scene):
        p = orc.shade_rays_paths(scene, rays, keys, eye, threads=THREADS)[0]
        c = orc.gather_rays(scene, rays, keys, eye, threads=THREADS)[0]
        a = orc.shade_rays_ambient(scene, rays, keys, c, eye, threads=THREADS)[0]
        assert same_bytes(a, p), "%s %s: AMBIENT(GATHER) differs from PATHS" % (tag, name)
        assert same_bytes(orc.shade_rays_ambient(scene, rays, keys, c[:, :3], eye, threads=THREADS)[0], p)  # (float32 [n, 3] too)
        junk = c.copy()
        junk[:, 3] = F("nan")
        assert same_bytes(orc.shade_rays_ambient(scene, rays, keys, junk, eye, threads=THREADS)[0], p), "the fourth float of amb is read"
        assert (c[:, :3] != 0).any()


@pytest.mark.parametrize("tag", ["p11x86_s1_120x90", "p11g_s2_160x90", "p13_p2_96x72"])
def test_ambient_of_zero_is_sampled_under_a_black_environment(pkg, orc, scenes, tag):
    scene, eye = scenes(tag), eye_of(scenes(tag))
    assert not scene.desc.environment.has_map and not any(scene.desc.environment.color)
    for name, rays, keys in family_k1(pkg, scene):
        s = orc.shade_rays_sampled(scene, rays, keys, eye, threads=THREADS)[0]
        for zero in (0.0, -0.0):
            amb = np.full((rays.size, 4), zero, F)
            assert same_bytes(orc.shade_rays_ambient(scene, rays, keys, amb, eye, threads=THREADS)[0], s), "%s %s amb %r" % (tag, name, zero)


# ---- independence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["p10_s4_160x120", "p13_p2_96x72"])
def test_the_answer_depends_on_ray_and_key_only(pkg, orc, scenes, tag):
    scene, eye = scenes(tag), eye_of(scenes(tag))
    _, rays, keys = family_k1(pkg, scene)[0]
    amb = np.random.RandomState(3).uniform(0, 1, (rays.size, 4)).astype(F)
    perm = np.random.RandomState(4).permutation(rays.size)
    cut = 777
    for mode in ("shade_rays_sampled", "shade_rays_paths", "gather_rays", "shade_rays_ambient"):
        def run(r, q, a, threads):
            args = (scene, r, q, a, eye) if mode == "shade_rays_ambient" else (scene, r, q, eye)
            return getattr(orc, mode)(*args, threads=threads)
        want, st = run(rays, keys, amb, 1)
        got8, st8 = run(rays, keys, amb, 8)
        assert same_bytes(got8, want) and st8 == st, mode + ": 8 threads"
        got, stp = run(rays[perm], keys[perm], amb[perm], 3)
        assert same_bytes(got, want[perm]) and stp == st, mode + ": a permutation"
        a, sa = run(rays[:cut], keys[:cut], amb[:cut], 2)
        b, sb = run(rays[cut:], keys[cut:], amb[cut:], 2)
        assert same_bytes(np.concatenate([a, b]), want) and {n: sa[n] + sb[n] for n in sa} == st, mode + ": a batch cut in two"
    # ... and on the key: other keys give other colours and the same t
    s0 = orc.shade_rays_paths(scene, rays, keys, eye, threads=THREADS)[0]
    s1 = orc.shade_rays_paths(scene, rays, keys ^ np.uint32(0x80000000), eye, threads=THREADS)[0]
    assert same_bytes(s0[:, 3], s1[:, 3]) and (bits(s0[:, :3]) != bits(s1[:, :3])).any(axis=1).sum() > 500


# ---- counters --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["p10_s4_160x120", "p11x86_s1_120x90"] + PATH_TAGS)
def test_counters_of_a_camera_batch_are_the_renders(pkg, orc, golden, scenes, tag):
    g, scene = golden(tag), scenes(tag)
    W, H = g.width, g.height
    frame = pkg.frame_setup(scene.desc.camera, W, H, samples=1)
    rays, keys = pkg.camera_sample_rays(frame, 0)
    eye = tuple(frame.cam_pos)
    _, want_s = orc.render_samples(scene, W, H, 1, threads=THREADS)
    _, want_p = orc.render_paths(scene, W, H, 1, threads=THREADS)
    _, got_s = orc.shade_rays_sampled(scene, rays, keys, eye, threads=THREADS)
    _, got_p = orc.shade_rays_paths(scene, rays, keys, eye, threads=THREADS)
    assert got_s == want_s and got_p == want_p
    assert got_s["primary_rays"] == W * H and got_p["shadow_rays"] > got_s["shadow_rays"] > 0
    # the two halves: together they count what PATHS counts, the primary rays twice
    c, st_g = orc.gather_rays(scene, rays, keys, eye, threads=THREADS)
    _, st_a = orc.shade_rays_ambient(scene, rays, keys, c, eye, threads=THREADS)
    for n in ("secondary_rays", "shadow_rays"):
        assert st_g[n] + st_a[n] == got_p[n], n
    assert st_g["primary_rays"] == st_a["primary_rays"] == W * H and st_g["primary_hits"] == st_a["primary_hits"] == got_p["primary_hits"]


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_and_accepted_scenes(pkg, orc, golden, scenes):
    scene = scenes("p10_s4_160x120")
    _, rays, keys = family_k1(pkg, scene)[0]
    r, q = np.ascontiguousarray(rays[:4]), np.ascontiguousarray(keys[:4])
    amb, out, eye = np.zeros((4, 4), F), np.zeros((4, 4), F), np.array(eye_of(scene), F)
    call = orc.lib.rtu_oracle_rays_keyed
    S, A = scene.desc_ptr, orc.KEYED_AMBIENT
    assert call(S, r.ctypes.data, q.ctypes.data, amb.ctypes.data, 4, eye.ctypes.data, A, out.ctypes.data, None, 1) == 0
    assert call(S, r.ctypes.data, None, amb.ctypes.data, 4, eye.ctypes.data, orc.KEYED_SAMPLED, out.ctypes.data, None, 1) == orc.ERR_ARG
    assert call(S, r.ctypes.data, q.ctypes.data, None, 4, eye.ctypes.data, A, out.ctypes.data, None, 1) == orc.ERR_ARG
    for mode in (orc.KEYED_SAMPLED, orc.KEYED_PATHS, orc.KEYED_GATHER):  # amb is read in AMBIENT only
        assert call(S, r.ctypes.data, q.ctypes.data, None, 4, eye.ctypes.data, mode, out.ctypes.data, None, 1) == 0
    assert call(S, None, q.ctypes.data, None, 4, eye.ctypes.data, orc.KEYED_PATHS, out.ctypes.data, None, 1) == orc.ERR_ARG
    assert call(S, r.ctypes.data, q.ctypes.data, None, 4, eye.ctypes.data, orc.KEYED_PATHS, None, None, 1) == orc.ERR_ARG
    assert call(S, r.ctypes.data, q.ctypes.data, None, 4, None, orc.KEYED_PATHS, out.ctypes.data, None, 1) == orc.ERR_ARG
    for mode in (-1, 4):
        assert call(S, r.ctypes.data, q.ctypes.data, amb.ctypes.data, 4, eye.ctypes.data, mode, out.ctypes.data, None, 1) == orc.ERR_ARG
    assert call(S, r.ctypes.data, q.ctypes.data, None, -1, eye.ctypes.data, orc.KEYED_PATHS, out.ctypes.data, None, 1) == orc.ERR_ARG
    assert call(None, r.ctypes.data, q.ctypes.data, None, 4, eye.ctypes.data, orc.KEYED_PATHS, out.ctypes.data, None, 1) == orc.ERR_ARG
    # n == 0: fine, whatever the pointers
    assert call(S, None, None, None, 0, eye.ctypes.data, A, None, None, 1) == 0
    assert orc.shade_rays_paths(scene, rays[:0], keys[:0], eye_of(scene))[0].shape == (0, 4)
    with pytest.raises(ValueError):
        orc.shade_rays_sampled(scene, rays, keys[:-1], eye_of(scene))
    # a scene without stochastic features is accepted, and SAMPLED is then recipe W under any key
    plain = golden("p4_240x135").scene(pkg)
    pr = family_b(pkg, "p4_240x135")[0][1]
    w = orc.shade_rays(plain, pr, eye_of(plain), threads=THREADS)
    s = orc.shade_rays_sampled(plain, pr, sample_keys(pkg, pr.size, 1), eye_of(plain), threads=THREADS)
    assert same_bytes(s[0], w[0]) and s[1] == w[1]
    # the unkeyed entry still refuses a stochastic scene
    with pytest.raises(orc.OracleError) as e:
        orc.trace_rays(scene, rays[:4])
    assert e.value.code == orc.ERR_STOCHASTIC


# ---- rtu_oracle_rays is what it was ----------------------------------------------------------------------------------------------
# SHA-256 of the answers to the second probe of family B in p4_240x135 (tests/test_oracle_rays.py), computed with the oracle as it
# stood before rtu_oracle_rays_keyed was added.
PINNED = {
    "closest": "7c39f59ecee4f817984b7237f3a4dd6c648819b7e10d15a7e6d5d79af437c230",
    "occluded": "f871e91fe7f660f598bd18f408e68c5bf76a305a4254dfa76980b1594bade52e",
    "shade": "5d62fd3a5b9e81dd553e479c2354f7f7174bd0712ee6d921f5db6bb8eb3d016b",
}


def test_the_unkeyed_entry_keeps_its_bytes(pkg, orc, golden):
    scene = golden("p4_240x135").scene(pkg)
    rays = family_b(pkg, "p4_240x135")[1][1]
    got = {"closest": orc.trace_rays(scene, rays, threads=3), "occluded": orc.occluded_rays(scene, rays, threads=3),
           "shade": orc.shade_rays(scene, rays, (3.0, -30.0, 9.0), threads=3, max_bounce=4)[0]}
    for name, a in got.items():
        assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() == PINNED[name], name


# ==== what the families hold ======================================================================================================
@pytest.fixture(scope="module")
def held(pkg, orc, scenes):
    """Per tag, once: {family: counts} of K1 (both probes together), K2 and K3."""
    cache = {}

    def get(tag):
        if tag not in cache:
            scene = scenes(tag)
            out = {}
            for fam, batches in (("K1", family_k1(pkg, scene)), ("K2", family_k2(pkg, orc, scene)), ("K3", family_k3(pkg, orc, scene))):
                total = {}
                for name, rays, keys in batches:
                    assert 0 < rays.size <= MAX_BATCH and valid(rays).all() and keys.dtype == np.uint32 and keys.size == rays.size
                    for n, v in contents(orc, scene, rays, keys).items():
                        total[n] = total.get(n, 0) + v
                print("%s %s: %s" % (tag, fam, total))
                out[fam] = total
            cache[tag] = out
        return cache[tag]
    return get


@pytest.mark.parametrize("tag", KEYED_TAGS)
def test_k1_probes_hold_chains_of_every_length(held, tag):
    c = held(tag)["K1"]
    assert c["rays"] == 2 * 64 * 33 and c["hits"] > 1000 and c["depth4"] >= 100
    if tag in OPEN_TAGS:
        assert c["misses"] >= 100 and all(c["leaves%d" % d] >= 30 for d in range(1, 5)), c
    else:
        assert c["misses"] == 0 and c["back"] >= 100, c  # the closed room: the probes see glass from inside instead
    if tag in SOFT_TAGS:
        assert c["partial"] >= 50, c
    if tag in GLOSSY_TAGS:
        assert c["glossy"] >= 50, c


@pytest.mark.parametrize("tag", KEYED_TAGS)
def test_k2_surface_starts_hold_back_faces(held, tag):
    c = held(tag)["K2"]
    assert c["hits"] >= 300 and c["back"] >= 30 and c["depth4"] >= 30, c
    if tag in OPEN_TAGS:
        assert c["misses"] >= 30, c
    if tag in SOFT_TAGS:
        assert c["partial"] >= 10, c


@pytest.mark.parametrize("tag", KEYED_TAGS)
def test_k3_keys_change_the_answer(pkg, orc, scenes, held, tag):
    scene, eye = scenes(tag), eye_of(scenes(tag))
    (_, rays, keys), = family_k3(pkg, orc, scene)
    c = held(tag)["K3"]
    assert c["rays"] == 64 and c["hits"] == 64 and c["back"] == 0
    first = {}
    for i, k in enumerate(keys):
        first.setdefault(int(k), i)
    again = np.array([first[int(k)] for k in keys])
    assert (again != np.arange(64)).sum() == 24
    for mode in (orc.shade_rays_sampled, orc.shade_rays_paths, orc.gather_rays):
        out = mode(scene, rays, keys, eye, threads=THREADS)[0]
        assert same_bytes(out, out[again]), "equal keys give other bytes"
        assert len(np.unique(out[:, 3])) == 1
        distinct = len(np.unique(out[:, :3], axis=0))
        print("%s %s: %d distinct colours under 40 keys" % (tag, mode.__name__, distinct))
        assert distinct >= (10 if mode is not orc.shade_rays_sampled else 2 if tag in SOFT_TAGS else 1)  # (a penumbra: lit or not)
    # a key that lost its top bit is another key
    g = orc.gather_rays(scene, rays, keys, eye, threads=THREADS)[0]
    g31 = orc.gather_rays(scene, rays, keys & np.uint32(0x7FFFFFFF), eye, threads=THREADS)[0]
    top = keys >= np.uint32(1 << 31)
    assert (bits(g[top, :3]) != bits(g31[top, :3])).any(axis=1).sum() >= 8 and same_bytes(g[~top], g31[~top])


@pytest.mark.parametrize("tag", list(SENSOR_TAGS))
def test_k4_sensor_rays_hit_miss_and_fall_outside(pkg, orc, scenes, tag):
    scene = scenes(tag)
    for model, d in k4_sensors(pkg, scene, SENSOR_TAGS[tag]):
        total = {}
        invalid = 0
        for k in range(SENSOR_SAMPLES):
            rays, keys = pkg.sensor_rays(d, k)
            ok = valid(rays)
            invalid += int((~ok).sum())
            assert rays.size == SENSOR_W * SENSOR_H and np.array_equal(keys, sample_keys(pkg, rays.size, k))
            for n, v in contents(orc, scene, rays[ok], keys[ok]).items():
                total[n] = total.get(n, 0) + v
        print("%s %s: %d invalid, %s" % (tag, model, invalid, total))
        assert total["hits"] >= 500 and total["depth4"] >= 100, total
        assert (invalid > 0) == (model == "fisheye")
        if model == "equirect":  # (the fisheye looks into the scene, the window lies inside it)
            assert total["misses"] >= 100, total
        if tag in SOFT_TAGS:
            assert total["partial"] >= 10, total


def test_k5_random_scenes_hold_what_the_golden_scenes_lack(pkg, orc, tmp_path_factory):
    from test_gpu_fuzz import write_assets
    assets = write_assets(tmp_path_factory.mktemp("keyed_fuzz"))
    total = {}
    for seed in S_SEEDS:
        scene = s_scene(pkg, assets, seed)
        seen = {}
        for name, rays, keys in family_k5(pkg, orc, scene, seed):
            assert 0 < rays.size <= FAMILY_SIZE and valid(rays).all()
            for n, v in contents(orc, scene, rays, keys).items():
                seen[n] = seen.get(n, 0) + v
        print("seed %d: %s" % (seed, seen))
        assert seen["hits"] >= 2000 and seen["back"] >= 100 and seen["misses"] >= 100, (seed, seen)
        for n, v in seen.items():
            total[n] = total.get(n, 0) + v
    print("K5, all seeds: %s" % total)
    assert total["glossy"] >= 1000 and total["partial"] >= 200 and all(total["leaves%d" % d] >= 200 for d in range(1, 5)) and total["depth4"] >= 1000, total


# ==== the irradiance map's chain on the oracle ====================================================================================
IRR_TAG = "p13_p2_96x72"
IRR_M, IRR_FIRST = 4, 3
# (width, height, min_subdiv, max_subdiv) -> the thresholds of the comparison of tests/test_gpu_irradiance.py, chosen here on the oracle's
# chain alone: both values of the byte plane occur, and no tested colour difference lies within IRR_MARGIN (relative) of its threshold
IRR_CASES = {(96, 72, -4, -1): dict(threshold_color=1.75, threshold_z=5.0, threshold_n=0.7),
             (24, 10, -3, -1): dict(threshold_color=1.0, threshold_z=20.0, threshold_n=0.7)}
IRR_COLOUR_BAR = 2e-4            # the bar E and the averages are held to on the device (tests/test_gpu_irradiance.py)
IRR_MARGIN = 10 * IRR_COLOUR_BAR


def oracle_irradiance_chain(pkg, orc, scene, case, thr, gather=None):
    """The host chain of test_the_device_build_is_the_host_chain with the oracle's trace and gather (or `gather(rays, keys)`): records,
    the byte plane, per pass (visited, computed), and the smallest relative distance of a tested colour difference |avg - E_i| to its
    threshold over all passes (every neighbour of every point a pass could estimate)."""
    W, H, mn, mx = case
    frame = pkg.frame_setup(scene.desc.camera, W, H)
    desc = pkg.irradiance_desc(min_subdiv=mn, max_subdiv=mx, samples=IRR_M, first_sample=IRR_FIRST, **thr)
    gw, gh, passes = pkg.irradiance_grid(desc, W, H)
    rays = pkg.irradiance_rays(frame, desc)
    eye = tuple(frame.cam_pos)
    hits = orc.trace_rays(plain_copy(pkg, scene), rays, threads=THREADS)
    if gather is None:
        gather = lambda r, q: orc.gather_rays(scene, r, q, eye, max_bounce=desc.max_bounce, threads=THREADS)[0]
    rec, comp = np.full((gh, gw, 8), F(-77.0), F), np.full((gh, gw), 9, np.uint8)
    tc = np.array(list(desc.threshold_color), np.float64)
    margin, per = np.inf, []
    for p in range(passes):
        phase, half, pts = pass_points(gw, gh, mx - mn, p)
        for x, y in pts:
            nb = neighbours(gw, gh, phase, half, x, y)
            if nb is None:
                continue
            d = [rec[b, a] for a, b in nb]
            avg = (((d[0] + d[1]) + d[2]) + d[3]) * F(0.25)
            for r in d:
                dif = np.abs(avg[:3] - r[:3]).astype(np.float64)
                margin = min(margin, float((np.abs(dif - tc) / tc).min()))
        visit, compute = pkg.irradiance_classify(desc, W, H, p, rec, comp)
        want = visit[compute]
        per.append((len(visit), len(want)))
        if len(want):
            r = np.repeat(rays[want], IRR_M)
            keys = np.array([pkg.sample_key(int(i), IRR_FIRST + m) for i in want for m in range(IRR_M)], np.uint32)
            c = gather(r, keys).reshape(len(want), IRR_M, 4)
            E = c[:, 0, :3].copy()
            for m in range(1, IRR_M):
                E = E + c[:, m, :3]  # float32, in the order of m
            E = E / F(IRR_M)
            flat = rec.reshape(-1, 8)
            flat[want, 0:3] = E
            flat[want, 3] = hits["t"][want]
            flat[want, 4:7] = hits["N"][want]
            flat[want, 7] = 0
            comp.reshape(-1)[want] = 1
            hit = (hits["flags"][want] & pkg.RTU_RAY_HIT) != 0
            flat[want[~hit], 4:7] = 0
    return SimpleNamespace(frame=frame, desc=desc, rays=rays, rec=rec, comp=comp, per=np.array(per, np.uint32), margin=margin, W=W, H=H, mx=mx)


@pytest.mark.parametrize("case", list(IRR_CASES), ids=lambda c: "%dx%d_%d_%d" % c)
def test_irradiance_thresholds_leave_a_margin(pkg, orc, scenes, case):
    b = oracle_irradiance_chain(pkg, orc, scenes(IRR_TAG), case, IRR_CASES[case])
    print("%dx%d: %d of %d points computed; per pass %s; the closest tested colour difference is %.3g of its threshold away from it"
          % (b.W, b.H, int(b.comp.sum()), b.comp.size, b.per.tolist(), b.margin))
    assert set(np.unique(b.comp)) == {0, 1}, "both values of the byte plane must occur"
    assert b.margin > IRR_MARGIN
