"""The inputs of the random-scene GPU tests, without a GPU: the scene generator pinned by hash, the ray families, the edit script and
the mesh deformations of tests/test_gpu_fuzz_rays.py and tests/test_gpu_fuzz_updates.py, each with the properties that make it worth
running (asserted on the oracle and on the host builders alone, as tests/test_oracle_rays.py does for its families).

  R1  rays from inside the object box, any direction: origins inside scaled groups, inside meshes, inside spheres
  R2  rays that start on surfaces, from R1's hit points along N, -N and the mirror direction
  R3  rays from a sphere around the scene, aimed into it; a third start under the 80-unit floor
  R4  R1's hit rays with tmax at the hit, one ulp before it, one ulp beyond it, and anywhere between half and one and a half of it

Everything is drawn from fixed seeds: the scenes from random.Random(1000 + seed) / (7000 + seed) as tests/test_gpu_fuzz.py draws them,
the rays from RandomState(5000 + seed), the edits from RandomState(9000 + seed)."""
import hashlib
import pathlib
import random

import numpy as np
import pytest

from test_gpu_fuzz import _make_stochastic, _scene_xml, write_assets
from test_gpu_ray_query import bits, nodes
from test_gpu_scene_update import RtuLight, lights, materials, mesh_nodes, shadow_lights
from test_mesh_update_host import RTU_MAX_BVH_STACK, clone, deform_name, deformed_scene
from test_oracle_rays import BIG, make_rays, renormalised, valid

W_SEEDS = range(24)
S_SEEDS = range(12)
TWO_MESH_SEEDS = [3, 5, 6, 8, 9, 10, 13, 15, 16, 18, 20, 21]
FAMILY_SIZE = 2048
EDIT_STEPS = 3
MESH_DEFORMATIONS = [("twist", 120), ("bulge", None), ("wobble", 2)]
RTU_OBJ_SPHERE, RTU_OBJ_PLANE, RTU_OBJ_TRIMESH = 1, 2, 3
RTU_LIGHT_DIRECT, RTU_LIGHT_POINT = 1, 2


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    return write_assets(tmp_path_factory.mktemp("fuzz_host"))


# ---- the scenes ------------------------------------------------------------------------------------------------------------------
def w_xml(seed, d):
    return _scene_xml(random.Random(1000 + seed), d, seed % 3 == 2)


def s_xml(seed, d):
    rnd = random.Random(7000 + seed)
    return _make_stochastic(_scene_xml(rnd, d, seed % 3 == 2), rnd)


def load(pkg, d, name, text):
    path = pathlib.Path(str(d)) / name
    path.write_text(text)
    return pkg.Scene.from_xml(str(path))


def w_scene(pkg, d, seed):
    """The scene of test_random_scene[seed]."""
    return load(pkg, d, "w%d.xml" % seed, w_xml(seed, d))


def s_scene(pkg, d, seed):
    """The scene of test_random_scene_sampled[seed]."""
    return load(pkg, d, "s%d.xml" % seed, s_xml(seed, d))


def eye_of(scene):
    return tuple(float(x) for x in scene.desc.camera.pos)


# SHA-256 of the XML text with "/fuzz" as the asset directory, of the generator as it stood when the ray, path and update tests were
# added: the scenes of the earlier tests must not move when the generator is extended (draw new things from another stream).
W_XML_SHA256 = [
    "cb77f11ab7041dc8dadc87f4654dcd8a870673545fa4b651922d21a128de855d",
    "3457f0eb0604c3cc79a27d2b67859ad03ea45e0d3644cfff3a067928909bc043",
    "fa0da1c5173d32dc0beb604f49a0e410012c5f230b35cd9faa34de1e9b39d26d",
    "d61bef64a841ac0cfa0c9f011f633385cf0a3a83054e4716ea8cbf3816d473d6",
    "033c7588870b16d4776705a58a671991c0706d70ef1d3328b212c5152442845f",
    "f0e3a24b1b22fc33c283bf75c19d14a96d49d8c8e2ca6b78c1d38e2b12494e1f",
    "cf39921140b70736476ac765897a4255dd2e8634bba51e48bfe160c5824f516b",
    "42d74cc10eb66865dc2b6112ed332f631f1d933229d3ae35f9ec02d316182905",
    "aecc48703cd7d1819afb034ce1ec1369fc2d91982617cf74c5f7d83f8cbc9e84",
    "8e7b957622a334ec2cdd5ed143aa0241ec55928903443c928571c2397c2feabb",
    "490d04574b0daaddccfd29c0c09459d1edff2c271f5e1e757ebfc5295d63604b",
    "37f40661f7dec864860ba721354fc65b83991cd2394d5e9976ecc78ee4ebe1de",
    "884d4a6f4455d136e220b059c6f93bed5d52100005edacfe018e7652006283bb",
    "23d97e11d165ec2c35b5eab33ef6d7a8e1e363187bcefe8d188cee9e7f190bf5",
    "725b3e4504aa937b6a74b161ab8f111f34a54d13494ed08646e56ebfc85c9390",
    "aa13b7d2176ed4abc44d7ca75c5a41059b3ec0691d7d8e08aae1fe0dd7bb505d",
    "9fc085578c224a86f3aaeccf38b2eda6a0310752227f5ec109badb0a4b935c11",
    "286f85ab97a7a8d42fdf6e11834a8ce823b75ee9a4b9b14f25fae8e2314d4ed4",
    "da020f7ef83bb5d7ca84b8ecdc8c11201fb47145ef7561854d90ca2560195938",
    "985f61a42ee2e729649bfc45d72c6d2e9ed11c970675b00cbaaf00edf6980ba2",
    "2b51e316d8969673dfece100801b5ad1d721655a350e66dcc71e28a33bd03f98",
    "00a5fe426e5fc8b96ed0f961ef3f2261a35e7558775c47a1f2dc87527e103831",
    "792e17e71c15c1de99d16972782c189cffe752f2fbfe120454634f40e7f807c5",
    "a0657b609086d58ad5b871dfdd1dfec6a067cf61b9af0705617ec8e73b280b1d",
]
S_XML_SHA256 = [
    "a791632cefeb084cfeccd210570f19de375cd730dbf8e85994056d647d206df7",
    "27e6d4c5ce5c19805b9d04686054659fbdaa455164cea52d26f4bbf741761d8f",
    "d935bcaf641795511052dc2591c1b85d4595f2a69c520bbcacbba0dff1e2bcda",
    "82638d95e7c235ed9a3384f7e27b3caeb03a5962b916c998e10e11d167719279",
    "24dcab0100ef56ff22c4a5f547a3cd88ae970f155e3fe153d0048db546cbaa34",
    "b022ff40fab1c942a1c0a80d336a4a600810c05da00e24498a9df7afd4575b08",
    "3504393dede0c96fbf9ee00ba32fd78666d6640218c77ac843e12ba03ecea84a",
    "35b496a2ace4afa71fe7fa18c5d0c60d24623d1a6f37965173305b2b21bdbf28",
    "a437dd3e5d15a06ce62f47ebdb57b426a0bfdd26f03ff5b3d81da46e6bc0efe1",
    "7667ad837fa464d1780e8a101878da75c2bee8a40d6f747513b6094d561d3434",
    "78f80eddeebcc08829bab035d35ad677e7bb8cc2826152a403ea16a6df82116a",
    "14a007ae6d114ead07398c430ab4bf8a77d40b63458630301701891de0eff435",
]


def test_the_generator_draws_the_scenes_it_drew():
    got_w = [hashlib.sha256(w_xml(seed, "/fuzz").encode()).hexdigest() for seed in W_SEEDS]
    got_s = [hashlib.sha256(s_xml(seed, "/fuzz").encode()).hexdigest() for seed in S_SEEDS]
    assert len(set(got_w + got_s)) == 36
    moved = [("W", i) for i in W_SEEDS if got_w[i] != W_XML_SHA256[i]] + [("S", i) for i in S_SEEDS if got_s[i] != S_XML_SHA256[i]]
    assert not moved, "the generator draws other scenes for %s" % moved


# ---- the ray families ------------------------------------------------------------------------------------------------------------
def family_r1(pkg, rng):
    """Inside: origins uniform in the box the objects are drawn in, directions uniform on the sphere."""
    org = rng.uniform((-9.0, -9.0, -5.0), (9.0, 9.0, 7.0), size=(FAMILY_SIZE, 3))
    return make_rays(pkg, org, renormalised(rng.normal(size=(FAMILY_SIZE, 3))))


def family_r2(pkg, r1, h1, hit):
    """Surface: from the hit points of R1 along N, -N and the mirror direction dir - 2 (dir . N) N; N renormalised twice in binary32."""
    p, N, d = h1["p"][hit], renormalised(h1["N"][hit]), r1["dir"][hit]
    k = np.float32(2) * ((d[:, 0] * N[:, 0] + d[:, 1] * N[:, 1]) + d[:, 2] * N[:, 2])
    return np.concatenate([make_rays(pkg, p, N), make_rays(pkg, p, -N), make_rays(pkg, p, renormalised(d - N * k[:, None]))])


def family_r3(pkg, rng):
    """Outside-in: origins on the sphere of radius 30 about the origin, every third one below z = -5 (under the floor) and the others
    above it, uniform by area in each band; each aimed at a point uniform in the middle of the object box."""
    n = FAMILY_SIZE
    under = np.arange(n) % 3 == 0
    z = np.where(under, rng.uniform(-1.0, -1.0 / 6.0, n), rng.uniform(-1.0 / 6.0, 1.0, n))
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    s = np.sqrt(1.0 - z * z)
    org = (30.0 * np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)).astype(np.float32)
    target = rng.uniform((-7.0, -7.0, -4.0), (7.0, 7.0, 5.0), size=(n, 3))
    return make_rays(pkg, org, renormalised(target - org.astype(np.float64)))


def family_r4(pkg, rng, r1, h1, hit):
    """tmax: R1's hit rays with tmax at the oracle's t, one ulp before it, one ulp beyond it, and uniform in (0.5 t, 1.5 t)."""
    base, t = r1[hit], h1["t"][hit]
    out = []
    for tmax in (t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(np.inf)), (t * rng.uniform(0.5, 1.5, t.size)).astype(np.float32)):
        r = base.copy()
        r["tmax"] = tmax
        out.append(r)
    return np.concatenate(out)


def ray_families(pkg, orc, scene, seed, trace=None):
    """[(name, rays)] of one W-seed, in the order R1, R2, R3, R4. R2 and R4 are built from the oracle's closest hits of R1 — or from
    those of trace(rays), where no oracle is at hand (tools/soak_fuzz.py)."""
    rng = np.random.RandomState(5000 + seed)
    r1 = family_r1(pkg, rng)
    h1 = orc.trace_rays(scene, r1, threads=8) if trace is None else trace(r1)
    hit = (h1["flags"] & pkg.RTU_RAY_HIT) != 0
    r3 = family_r3(pkg, rng)
    fam = [("R1 inside", r1), ("R2 surface", family_r2(pkg, r1, h1, hit)), ("R3 outside-in", r3), ("R4 tmax", family_r4(pkg, rng, r1, h1, hit))]
    for _, rays in fam:
        rays.setflags(write=False)
    return fam


def kinds_of(scene):
    nd = nodes(scene)
    return np.array([nd[i].obj_type for i in range(scene.desc.n_nodes)], np.int32)


@pytest.fixture(scope="module")
def traced(pkg, orc, assets):
    """Per W-seed, once: (the families, per family (rays, hits, back-face hits), kinds of object present, kinds hit)."""
    cache = {}

    def get(seed):
        if seed not in cache:
            scene = w_scene(pkg, assets, seed)
            kinds = kinds_of(scene)
            fam = dict(ray_families(pkg, orc, scene, seed))
            fig, seen = {}, set()
            for name, rays in fam.items():
                assert 0 < rays.size <= 4 * FAMILY_SIZE and valid(rays).all(), "%s: %d invalid rays" % (name, int((~valid(rays)).sum()))
                h = orc.trace_rays(scene, rays, threads=8)
                hit = (h["flags"] & orc.RAY_HIT) != 0
                back = hit & ((h["flags"] & orc.RAY_FRONT) == 0)
                fig[name] = (rays.size, int(hit.sum()), int(back.sum()))
                seen |= set(int(k) for k in np.unique(kinds[h["node"][hit]]))
                print("seed %d %s: %d rays, %d hit, %d of them a back face" % ((seed, name) + fig[name]))
            t1 = orc.trace_rays(scene, fam["R1 inside"], threads=8)["t"]
            cache[seed] = (fam, fig, set(int(k) for k in kinds if k != 0), seen, t1)
        return cache[seed]
    return get


@pytest.mark.parametrize("seed", W_SEEDS)
def test_ray_families_contain_what_they_are_for(traced, seed):
    fam, fig, _, _, t = traced(seed)
    assert sorted(fam) == ["R1 inside", "R2 surface", "R3 outside-in", "R4 tmax"]
    n, hit, back = fig["R1 inside"]
    assert n == FAMILY_SIZE and hit >= 0.25 * n and n - hit >= 0.10 * n and back >= 0.01 * n
    assert fig["R2 surface"][0] == 3 * hit and fig["R4 tmax"][0] == 4 * hit
    n, hit, back = fig["R3 outside-in"]
    assert n == FAMILY_SIZE and hit >= 0.80 * n and back >= 0.20 * n
    org = fam["R3 outside-in"]["org"]
    assert abs(int((org[:, 2] < -5.0).sum()) - n / 3.0) < 1.0 and np.all(np.abs(np.linalg.norm(org.astype(np.float64), axis=1) - 30.0) < 1e-4)
    n, hit, _ = fig["R2 surface"]
    assert hit >= 0.05 * n
    # R4: a quarter each, in the order at the hit, one ulp before it, one ulp beyond it, around it
    r4, t = fam["R4 tmax"], t[t != BIG]
    q = r4.size // 4
    assert np.array_equal(bits(r4["tmax"][:q]), bits(t)) and np.all(r4["tmax"][q:2 * q] < t) and np.all(r4["tmax"][2 * q:3 * q] > t)
    assert np.all(r4["tmax"][3 * q:] >= np.float32(0.5) * t) and np.all(r4["tmax"][3 * q:] <= np.float32(1.5) * t)


def test_every_object_kind_is_hit_over_the_seeds(traced):
    present = set().union(*(traced(seed)[2] for seed in W_SEEDS))
    seen = set().union(*(traced(seed)[3] for seed in W_SEEDS))
    assert present == {RTU_OBJ_SPHERE, RTU_OBJ_PLANE, RTU_OBJ_TRIMESH} and seen == present


# ---- the edit script -------------------------------------------------------------------------------------------------------------
def edit_step(pkg, scene, rng):
    """One step of the script, applied to `scene` in place. Every node but the root, independently: translated by up to +-2 along each
    axis (probability 0.5), turned about an axis drawn from a normal distribution by up to +-40 degrees (0.5), scaled per axis by 0.6 to 1.6
    (0.3). Every point light moves to a point uniform in (-9, -9, -3) ... (9, 9, 12), into the object box as well; every direct light gets a
    direction uniform in (-1, -1, -1) ... (1, 1, -0.02), grazing ones included. One material's diffuse colour changes."""
    nd = nodes(scene)
    for i in range(scene.desc.n_nodes):
        if nd[i].parent < 0:
            continue
        if rng.uniform() < 0.5:
            scene.node_translate(i, tuple(float(x) for x in rng.uniform(-2.0, 2.0, 3)))
        if rng.uniform() < 0.5:
            scene.node_rotate(i, tuple(float(x) for x in rng.normal(size=3)), float(rng.uniform(-40.0, 40.0)))
        if rng.uniform() < 0.3:
            scene.node_scale(i, *(float(x) for x in rng.uniform(0.6, 1.6, 3)))
    for i in range(scene.desc.n_lights):
        nl = RtuLight.from_buffer_copy(bytes(lights(scene)[i]))
        if nl.type == RTU_LIGHT_POINT:
            nl.vec[0], nl.vec[1], nl.vec[2] = (float(x) for x in rng.uniform((-9.0, -9.0, -3.0), (9.0, 9.0, 12.0)))
        elif nl.type == RTU_LIGHT_DIRECT:
            nl.vec[0], nl.vec[1], nl.vec[2] = (float(x) for x in rng.uniform((-1.0, -1.0, -1.0), (1.0, 1.0, -0.02)))
        else:
            continue
        scene.set_light(i, nl)
    m = materials(scene)[int(rng.randint(scene.desc.n_materials))]
    m.diffuse[0], m.diffuse[1], m.diffuse[2] = (float(x) for x in rng.uniform(0.0, 1.0, 3))


def edit_script(pkg, scene, seed):
    """The EDIT_STEPS chained scenes of one seed: each a clone of the one before it, edited."""
    rng = np.random.RandomState(9000 + seed)
    out = []
    for _ in range(EDIT_STEPS):
        scene = clone(pkg, scene)
        edit_step(pkg, scene, rng)
        out.append(scene)
    return out


def list_pairs(pkg, scene):
    """(usable, unusable) pairs of (shadow light, mesh node) of the host builder, over the pairs assert_lists_equal looks at."""
    usable = unusable = 0
    for ls in range(min(len(shadow_lights(scene)), 4)):
        for cs in range(len(mesh_nodes(scene))):
            if pkg.light_list(scene, ls, cs) is None:
                unusable += 1
            else:
                usable += 1
    return usable, unusable


def test_the_edit_script_gives_the_list_builder_work(pkg, assets):
    usable = unusable = 0
    with_unusable = []
    for seed in W_SEEDS:
        scene = w_scene(pkg, assets, seed)
        blob = scene.to_blob_bytes()
        for step, now in enumerate(edit_script(pkg, scene, seed)):
            assert pkg.scene_shape_diff(scene, now) is None  # an update takes it
            assert now.to_blob_bytes() != blob
            blob = now.to_blob_bytes()
            u, n = list_pairs(pkg, now)
            usable, unusable = usable + u, unusable + n
            if n:
                with_unusable.append((seed, step))
    print("edit script: %d usable and %d unusable (light, mesh node) pairs; unusable at (seed, step) %s" % (usable, unusable, with_unusable))
    assert usable >= 100 and unusable >= 5


# ---- the mesh deformations -------------------------------------------------------------------------------------------------------
def mesh_script(pkg, scene):
    """[(scene, mesh ids, name)]: mesh 0 twisted, then mesh 1 bulged as well, then both wobbled on top — the chain the refit follows."""
    (d0, d1, d2), out = MESH_DEFORMATIONS, []
    now = deformed_scene(pkg, scene, 0, d0)
    out.append((now, [0], "%s of mesh 0" % deform_name(d0)))
    now = deformed_scene(pkg, now, 1, d1)
    out.append((now, [1], "%s of mesh 1" % deform_name(d1)))
    now = deformed_scene(pkg, deformed_scene(pkg, now, 0, d2), 1, d2)
    out.append((now, [0, 1], "%s of both" % deform_name(d2)))
    return out


def test_the_seeds_with_two_meshes(pkg, assets):
    two = [seed for seed in W_SEEDS if w_scene(pkg, assets, seed).desc.n_meshes == 2]
    assert two == TWO_MESH_SEEDS
    for seed in two:  # a property of these inputs (rtu_update_meshes needs it), not a skip
        scene = w_scene(pkg, assets, seed)
        assert len(mesh_nodes(scene)) >= 2
        for now, meshes, name in mesh_script(pkg, scene):
            assert all(now.mesh(m).bvh_depth <= RTU_MAX_BVH_STACK for m in (0, 1)), "seed %d, %s" % (seed, name)


@pytest.mark.parametrize("seed", [3, 15, 18])
def test_mesh_deformations_change_the_image(pkg, orc, assets, seed):
    scene = w_scene(pkg, assets, seed)
    W, H = 96, 64
    base = orc.render(scene, W, H, threads=8)[0]
    for meshes in ([0], [1], [0, 1]):
        for d in MESH_DEFORMATIONS:
            now = scene
            for m in meshes:
                now = deformed_scene(pkg, now, m, d)
            img = orc.render(now, W, H, threads=8)[0]
            changed = int((bits(img) != bits(base)).any(axis=-1).sum())
            print("seed %d, %s of mesh %s: %d pixels change" % (seed, deform_name(d), meshes, changed))
            assert changed > 0
    prev = base
    for now, meshes, name in mesh_script(pkg, scene):
        img = orc.render(now, W, H, threads=8)[0]
        assert (bits(img) != bits(prev)).any(), "seed %d: %s changes no pixel" % (seed, name)
        prev = img
