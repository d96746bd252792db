"""rtu_shade_rays_sampled, rtu_shade_rays_paths, rtu_gather_rays and rtu_shade_rays_ambient (host forms) against the oracle's keyed
ray-level entry (rtu_oracle_rays_keyed) on rays no camera fires and keys no pixel has: the families of tests/test_oracle_rays_keyed.py,
which asserts on the oracle alone that each contains what it is meant to.

  K1  equirectangular probes from two points inside the scene
  K2  rays that start on surfaces along N, -N and the mirror direction: root hits on back faces, from inside
  K3  one hit ray 64 times under keys from the corners of the 32-bit range, child keys, sample keys; equal keys at two indices
  K4  the rays of a fisheye, a panoramic and an orthographic sensor, sample by sample, and the sensor's image
  K5  the families R1-R4 of tests/test_fuzz_host.py on the twelve stochastic random scenes

Every batch goes through check_keyed_batch, the counterpart of check_batch in tests/test_gpu_rays_oracle.py. Exact: t (the oracle's
and rtu_trace_rays'), hit and miss, NaN masks, the counters, sixteen zero bytes for an invalid ray, the environment's bytes and tmax at a
miss, the counting variant's and a sorted batch's bytes. Colours: the bar of check() in tests/test_gpu_shade_rays_sampled.py (8-bit +-1,
linear 2e-4) on the golden scenes; where a ray can start inside glass (K2, K5) INSIDE_GLASS_REL_TOL of tests/test_gpu_fuzz.py over
recipe S's floor 1e-3 and recipe P's 1e-2 (NOTEBOOK section 18 says why). The gathered light c, a quantity no earlier test held
against the oracle, takes recipe P's bar of the scene's class; NOTEBOOK section 20 has the measured maxima per family."""
import numpy as np
import pytest

from test_gpu_fuzz import INSIDE_GLASS_REL_TOL, assets, check_paths  # noqa: F401  (assets: the fixture)
from test_gpu_parity import check_against
from test_gpu_ray_query import bits
from test_gpu_shade_rays_sampled import check, environment_of, same_bytes
from test_fuzz_host import S_SEEDS, s_scene
from test_oracle_rays_keyed import (KEYED_TAGS, MAX_BATCH, SENSOR_SAMPLES, SENSOR_TAGS, THREADS, eye_of, family_k1, family_k2, family_k3,
                                    family_k5, k4_sensors)
from test_oracle_rays import BIG, valid

pytestmark = pytest.mark.gpu

F = np.float32
ENTRIES = ("sampled", "paths", "gather", "ambient")
GOLDEN_ABS_TOL = 2e-4  # check()'s linear bar, for c on the golden scenes


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def colours_within(out, cpu, orc, entry, inside_glass, what):
    """The colour bar of one entry's answer (float32 [n, 4], t equal already). NaN colours are results like any other: at the same
    rays on both sides, the rest compared by value. Prints the largest deviation before it asserts."""
    nan = np.isnan(cpu[:, :3])
    assert np.array_equal(np.isnan(out[:, :3]), nan), what + ": NaN colours at different rays"
    a, b = np.where(nan, F(0), out[:, :3]), np.where(nan, F(0), cpu[:, :3])
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    rel = d / np.maximum(np.abs(b.astype(np.float64)), 1e-3 if entry == "sampled" else 1e-2)
    worst = int(np.argmax(rel.max(axis=1)))
    print("%s: %d NaN colours; largest |difference| %.3g, largest relative %.3g (ray %d, oracle %s), largest |value| %.3g"
          % (what, int(nan.any(axis=1).sum()), d.max(), rel.max(), worst, cpu[worst, :3].tolist(), np.abs(b).max()))
    g, c = np.concatenate([a, out[:, 3:]], axis=1).reshape(1, -1, 4), np.concatenate([b, cpu[:, 3:]], axis=1).reshape(1, -1, 4)
    if entry == "gather":  # a light's intensity, no pixel: the linear bars alone
        if inside_glass:
            assert rel.max() < INSIDE_GLASS_REL_TOL, "%s: c differs by %.3g of max(|value|, 1e-2)" % (what, rel.max())
        else:
            assert d.max() < GOLDEN_ABS_TOL, "%s: c differs by %.3g" % (what, d.max())
    elif not inside_glass:
        check(g, c, orc, 1, what)
    elif entry == "sampled":
        check_against(g, c, orc, rel_tol=INSIDE_GLASS_REL_TOL)
    else:
        check_paths(g, c, orc, what)


def check_keyed_batch(pkg, orc, ctx, scene, rays, keys, eye, label, entries=ENTRIES, inside_glass=False, max_bounce=5):
    """One batch (the scene is uploaded) through the host forms of `entries` against the oracle. Rays the header calls invalid are not
    given to the oracle: they must come back as sixteen zero bytes. Returns {entry: the device's answer} and the hit mask."""
    assert 0 < rays.size <= MAX_BATCH and keys.dtype == np.uint32 and keys.size == rays.size
    ok = valid(rays)
    r_ok, k_ok = np.ascontiguousarray(rays[ok]), np.ascontiguousarray(keys[ok])
    traced = ctx.trace_rays(rays)
    assert np.array_equal((traced["flags"] & pkg.RTU_RAY_INVALID) != 0, ~ok)
    hit = (traced["flags"] & pkg.RTU_RAY_HIT) != 0
    miss = ok & ~hit
    env = environment_of(pkg, ctx, scene, rays["dir"][miss]) if miss.any() else None
    cpu_c = np.zeros((rays.size, 4), F)  # the oracle's gathered light: what AMBIENT is given on both sides
    cpu_c[ok] = orc.gather_rays(scene, r_ok, k_ok, eye, max_bounce=max_bounce, threads=THREADS)[0]
    outs = {}
    for entry in entries:
        what = "%s %s" % (label, entry)
        cpu = np.zeros((rays.size, 4), F)
        if entry == "sampled":
            cpu[ok], cstats = orc.shade_rays_sampled(scene, r_ok, k_ok, eye, max_bounce=max_bounce, threads=THREADS)
            run = lambda **kw: ctx.shade_rays_sampled(rays, keys, eye, max_bounce=max_bounce, **kw)
        elif entry == "paths":
            cpu[ok], cstats = orc.shade_rays_paths(scene, r_ok, k_ok, eye, max_bounce=max_bounce, threads=THREADS)
            run = lambda **kw: ctx.shade_rays_paths(rays, keys, eye, max_bounce=max_bounce, **kw)
        elif entry == "gather":
            cpu[ok], cstats = cpu_c[ok], orc.gather_rays(scene, r_ok, k_ok, eye, max_bounce=max_bounce, threads=THREADS)[1]
            run = lambda **kw: ctx.gather_rays(rays, keys, eye, max_bounce=max_bounce, **kw)
        else:
            cpu[ok], cstats = orc.shade_rays_ambient(scene, r_ok, k_ok, cpu_c[ok], eye, max_bounce=max_bounce, threads=THREADS)
            run = lambda **kw: ctx.shade_rays_ambient(rays, keys, cpu_c, eye, max_bounce=max_bounce, **kw)
        out = run()[0]  # the fast variant first: it sizes the frame records the counting variant needs
        tbad = int((bits(out[:, 3]) != bits(cpu[:, 3])).sum())
        print("%s: %d rays (%d valid), %d hit; t differs from the oracle's at %d" % (what, rays.size, int(ok.sum()), int(hit.sum()), tbad))
        assert tbad == 0, what + ": t differs from the oracle's"
        assert np.array_equal(bits(out[:, 3]), bits(traced["t"] * ok)), what + ": t differs from rtu_trace_rays"  # (an invalid ray: t = 0)
        assert not out[~ok].view(np.uint8).any(), what + ": an invalid ray must give sixteen zero bytes"
        if miss.any():
            assert np.array_equal(bits(out[miss, 3]), bits(rays["tmax"][miss])), what + ": a miss must return tmax"
            if entry == "gather":
                assert not out[miss, :3].view(np.uint32).any(), what + ": a miss gathers nothing"
            else:
                assert same_bytes(out[miss, :3], env), what + ": a miss must be the environment along the ray"
        colours_within(out, cpu, orc, entry, inside_glass, what)
        ref, stats = run(reference_walk=True, stats=True)
        assert same_bytes(ref, out), what + ": the counting variant's bytes differ from the fast variant's"
        assert stats == cstats, "%s: counters differ from the oracle's: %s vs %s" % (what, stats, cstats)
        if entry in ("sampled", "paths"):
            assert same_bytes(run(sort=True)[0], out), what + ": a sorted batch gives other bytes"
        outs[entry] = out
    return outs, hit


@pytest.fixture(scope="module")
def scenes(pkg, golden):
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = golden(tag).scene(pkg)
        return cache[tag]
    return get


# ---- K1 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", KEYED_TAGS)
def test_k1_probes(pkg, orc, ctx, scenes, tag):
    scene = scenes(tag)
    ctx.upload(scene)
    for name, rays, keys in family_k1(pkg, scene):
        check_keyed_batch(pkg, orc, ctx, scene, rays, keys, eye_of(scene), "K1 %s %s" % (tag, name))


def test_k1_probes_another_eye_and_depth(pkg, orc, ctx, scenes):
    scene = scenes("p10_s4_160x120")
    ctx.upload(scene)
    name, rays, keys = family_k1(pkg, scene)[0]
    check_keyed_batch(pkg, orc, ctx, scene, rays, keys, (3.0, -30.0, 9.0), "K1 p10 %s, eye (3, -30, 9), max_bounce 2" % name, max_bounce=2)


# ---- K2 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", KEYED_TAGS)
def test_k2_surface_starts(pkg, orc, ctx, scenes, tag):
    scene = scenes(tag)
    ctx.upload(scene)
    for name, rays, keys in family_k2(pkg, orc, scene):
        check_keyed_batch(pkg, orc, ctx, scene, rays, keys, eye_of(scene), "K2 %s %s" % (tag, name), inside_glass=True)


# ---- K3 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", KEYED_TAGS)
def test_k3_keys(pkg, orc, ctx, scenes, tag):
    scene = scenes(tag)
    ctx.upload(scene)
    (name, rays, keys), = family_k3(pkg, orc, scene)
    outs, hit = check_keyed_batch(pkg, orc, ctx, scene, rays, keys, eye_of(scene), "K3 %s %s" % (tag, name))
    assert hit.all()
    first = {}
    for i, k in enumerate(keys):
        first.setdefault(int(k), i)
    again = np.array([first[int(k)] for k in keys])
    assert (again != np.arange(keys.size)).sum() == 24
    for entry, out in outs.items():
        assert same_bytes(out, out[again]), "K3 %s %s: equal keys give other bytes" % (tag, entry)


# ---- K4 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(SENSOR_TAGS))
def test_k4_sensors(pkg, orc, ctx, scenes, tag):
    scene = scenes(tag)
    ctx.upload(scene)
    gather = SENSOR_TAGS[tag]
    entries = ("paths", "gather", "ambient") if gather else ("sampled",)
    for model, d in k4_sensors(pkg, scene, gather):
        eye = tuple(d.pos)
        pixels = d.width * d.height
        s, zs, nh = np.zeros((pixels, 3), F), np.zeros(pixels, F), np.zeros(pixels, np.uint32)
        for k in range(SENSOR_SAMPLES):
            rays, keys = pkg.sensor_rays(d, k)
            check_keyed_batch(pkg, orc, ctx, scene, rays, keys, eye, "K4 %s %s sample %d" % (tag, model, k), entries=entries)
            ok = valid(rays)
            cpu = np.zeros((pixels, 4), F)
            entry = orc.shade_rays_paths if gather else orc.shade_rays_sampled
            cpu[ok] = entry(scene, np.ascontiguousarray(rays[ok]), np.ascontiguousarray(keys[ok]), eye, threads=THREADS)[0]
            s += cpu[:, :3]  # binary32, in sample order
            hit = ok & (cpu[:, 3] != BIG)
            zs[hit] += cpu[hit, 3]
            nh[hit] += 1
        want = np.empty((pixels, 4), F)
        want[:, :3] = s / F(SENSOR_SAMPLES)
        with np.errstate(all="ignore"):
            want[:, 3] = np.where(nh > 0, zs / nh.astype(F), BIG)
        got = ctx.render_sensor(d).reshape(-1, 4)
        ctx.frame_status()
        assert np.array_equal(bits(got[:, 3]), bits(want[:, 3])), "K4 %s %s: the image's z differs from the oracle's samples" % (tag, model)
        colours_within(got, want, orc, "paths" if gather else "sampled", False, "K4 %s %s image" % (tag, model))


# ---- K5 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", S_SEEDS)
def test_k5_random_scene_rays(pkg, orc, ctx, assets, seed):  # noqa: F811
    scene = s_scene(pkg, assets, seed)
    ctx.upload(scene)
    for name, rays, keys in family_k5(pkg, orc, scene, seed):
        _, hit = check_keyed_batch(pkg, orc, ctx, scene, rays, keys, eye_of(scene), "K5 seed %d %s" % (seed, name),
                                   entries=("sampled", "paths", "gather"), inside_glass=True)
        assert hit.any()
