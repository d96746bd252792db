"""rtu_trace_rays, rtu_occluded_rays and rtu_shade_rays against the oracle's ray-level entry (rtu_oracle_rays) on rays no camera
fires: the families of tests/test_oracle_rays.py, which asserts on the oracle alone that each contains what it is meant to.

  A  orthographic grids with axis-parallel directions (exact zeros, +0.0 and -0.0), origins in the planes of the reference's boxes
  B  panoramic probes from inside the scene: exact poles, an exact equator, sphere centres, NaN colours of the reference
  C  tmax at, one ulp beyond and one ulp before the hit; between the first and the second hit
  D  rays that start on surfaces, along N, -N and the mirror direction
  E  directions across the accepted unit-length band

The bars are the same for every batch (check_batch): every field of a closest hit equal to the oracle's, t / p / N bit for bit; the
occlusion byte equal; the radiance with t bit-exact, colours within the project's bar (check_against: NaN at the same rays, 8-bit
+-1, linear relative error <= 2e-5) and the counters equal; the reference walk byte-identical to the fast walk in all three."""
import numpy as np
import pytest

from test_gpu_parity import RGB_REL_TOL, check_against
from test_gpu_ray_query import bits, nodes, same_hits
from test_oracle_rays import (A1_BATCH, BIG, PROBES, axis_scene, family_a1, family_a2, family_a3, family_b, family_c, family_d,
                              family_e, frame_of, make_rays, valid)

pytestmark = pytest.mark.gpu

MAX_CALL = 30000


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def ulp_distance(a, b):
    """Largest distance in units of the last place between two float32 arrays (0 where the bits agree)."""
    def ordered(x):
        i = bits(x).astype(np.int64)
        return np.where(i & 0x80000000, 0x80000000 - i, i)
    d = np.abs(ordered(a) - ordered(b))
    return int(d.max()) if d.size else 0


def check_batch(pkg, orc, ctx, scene, rays, eye, label, max_bounce=5, rel_tol=RGB_REL_TOL):
    """One batch (the scene is uploaded) against the oracle in all three forms and both walks. Rays the header calls invalid are
    not given to the oracle: they must come back flagged, as a miss, not occluded, sixteen zero bytes. rel_tol: the bar of the linear
    colours (check_against). Returns the hit mask."""
    assert 0 < rays.size <= MAX_CALL
    ok = valid(rays)
    n_ok = int(ok.sum())
    # ---- closest hit
    want = np.zeros(rays.size, pkg.hit_dtype())
    want["t"], want["node"], want["material"], want["flags"] = rays["tmax"], -1, -1, pkg.RTU_RAY_INVALID
    want[ok] = orc.trace_rays(scene, rays[ok], threads=8)
    got = ctx.trace_rays(rays)
    hit = (want["flags"] & pkg.RTU_RAY_HIT) != 0
    bad = {f: int((bits(got[f]) != bits(want[f])).sum()) for f in ("t", "flags", "node", "material")}
    bad_p, bad_n = int((bits(got["p"]) != bits(want["p"])).any(axis=1).sum()), int((bits(got["N"]) != bits(want["N"])).any(axis=1).sum())
    print("%s: %d rays (%d valid), %d hits; differing from the oracle: %s, p %d (largest %d ulp), N %d (largest %d ulp)" %
          (label, rays.size, n_ok, int(hit.sum()), bad, bad_p, ulp_distance(got["p"], want["p"]), bad_n, ulp_distance(got["N"], want["N"])))
    assert not any(bad.values()), "closest hit differs from the oracle: %s" % bad
    assert bad_p == 0 and bad_n == 0, "hInfo.p / hInfo.N differ from the oracle's"
    miss = ~hit
    assert np.all(got["node"][miss] == -1) and np.all(got["material"][miss] == -1) and not got["p"][miss].any() and not got["N"][miss].any()
    assert np.array_equal(bits(got["t"][miss]), bits(rays["tmax"][miss])) and np.all(got["flags"][miss & ok] == 0)
    assert not got["pad0"].any() and not got["pad1"].any()
    assert same_hits(ctx.trace_rays(rays, reference_walk=True), got), "the reference walk's closest hits differ from the fast walk's"
    # ---- occlusion
    occ = np.zeros(rays.size, np.uint8)
    occ[ok] = orc.occluded_rays(scene, rays[ok], threads=8)
    for ref in (False, True):
        o = ctx.occluded(rays, reference_walk=ref)
        wrong = int((o != occ).sum())
        print("%s ref=%s: %d occluded, %d bytes differ from the oracle's" % (label, ref, int(occ.sum()), wrong))
        assert wrong == 0
    # ---- radiance
    cpu = np.zeros((rays.size, 4), np.float32)
    cpu[ok], cstats = orc.shade_rays(scene, rays[ok], eye, threads=8, max_bounce=max_bounce)
    out = ctx.shade_rays(rays, eye, max_bounce=max_bounce)[0]
    tbad = int((bits(out[:, 3]) != bits(cpu[:, 3])).sum())
    nan = np.isnan(cpu[:, :3]).any(axis=1)
    print("%s: shade t differs at %d rays; %d NaN colours in the oracle's answer" % (label, tbad, int(nan.sum())))
    assert tbad == 0
    assert np.array_equal(bits(out[:, 3]), bits(got["t"] * ok))  # (an invalid ray: t = 0)
    assert not out[~ok].view(np.uint8).any(), "an invalid ray must give sixteen zero bytes"
    with np.errstate(invalid="ignore"):
        rel = np.abs(out[:, :3].astype(np.float64) - cpu[:, :3]) / np.maximum(np.abs(cpu[:, :3].astype(np.float64)), 1e-3)
    print("%s: linear RGB differs by at most %.3g of max(|value|, 1e-3)" % (label, np.nanmax(rel) if np.isfinite(rel).any() else 0.0))
    check_against(out.reshape(1, -1, 4), cpu.reshape(1, -1, 4), orc, rel_tol=rel_tol)
    ref, stats = ctx.shade_rays(rays, eye, max_bounce=max_bounce, reference_walk=True, stats=True)
    assert np.array_equal(ref.view(np.uint8), out.view(np.uint8)), "the counting variant's radiance differs from the fast variant's"
    assert stats == cstats, "counters differ from the oracle's: %s vs %s" % (stats, cstats)
    return hit


def eye_of(scene):
    return tuple(float(x) for x in scene.desc.camera.pos)


# ---- family A --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def axis(pkg, golden):
    return axis_scene(pkg, golden)


def test_axis_scene_uploads_as_edited(pkg, orc, ctx, axis):
    """AXIS is made by editing the node of a loaded scene: what the device holds is that scene (its camera rays give the oracle's z)."""
    ctx.upload(axis)
    cam = axis.desc.camera
    frame = frame_of(pkg, axis, cam.img_width, cam.img_height)
    rays = pkg.camera_rays(frame, 20, 100)
    z = orc.render(axis, cam.img_width, cam.img_height, threads=8, row0=20, nrows=100)[0][..., 3].reshape(-1)
    assert (z != BIG).sum() > 1000 and np.array_equal(bits(ctx.render(frame)[0][20:120, :, 3].reshape(-1)), bits(z))
    check_batch(pkg, orc, ctx, axis, rays, tuple(frame.cam_pos), "AXIS camera rows 20-119")


@pytest.mark.parametrize("k", [0, 1, 2])
def test_a1_rays_in_the_planes_of_the_reference_boxes(pkg, orc, ctx, axis, k):
    ctx.upload(axis)
    fam = family_a1(pkg, axis)[4 * k:4 * k + 4]  # +e_k and -e_k, zeros +0.0 and -0.0
    for name, rays in fam:
        assert name[1] == "xyz"[k] and rays.size == A1_BATCH
        hit = check_batch(pkg, orc, ctx, axis, rays, eye_of(axis), "A1 " + name)
        assert hit.any() and not hit.all()


@pytest.mark.parametrize("name", ["AXIS", "ties_160x120"])
def test_a2_single_zero_directions(pkg, orc, ctx, golden, axis, name):
    scene = axis if name == "AXIS" else golden(name).scene(pkg)
    ctx.upload(scene)
    for what, rays in family_a2(pkg, name):
        hit = check_batch(pkg, orc, ctx, scene, rays, eye_of(scene), "A2 %s %s" % (name, what))
        assert hit.any() and not hit.all()


@pytest.mark.parametrize("tag", ["p4_240x135", "teapot2_240x135"])
def test_a3_rays_in_the_faces_of_sphere_boxes(pkg, orc, ctx, golden, tag):
    scene = golden(tag).scene(pkg)
    ctx.upload(scene)
    for what, rays in family_a3(pkg, scene, tag):
        hit = check_batch(pkg, orc, ctx, scene, rays, eye_of(scene), "A3 %s %s" % (tag, what))
        assert hit.any() and not hit.all()


def test_hits_in_the_edge_zone_of_a_plane(pkg, orc, ctx, golden):
    """A plane hit within 1e-5 (1 + |p|) of an edge of the unit square takes the box test of the fast plane form. Family A1 found one
    such ray whose p lost a component (the closest-hit kernels had been compiled wrongly there); here 16 rays
    along each of the four edges of teapot2's floor, 1.2e-5 inside it, and 16 through its interior, straight down, obliquely and
    from below."""
    scene = golden("teapot2_240x135").scene(pkg)
    ctx.upload(scene)
    n = nodes(scene)[2]
    assert n.obj_type == 2  # RTU_OBJ_PLANE
    tm, pos = np.array(list(n.tm), np.float64).reshape(3, 3).T, np.array(list(n.pos), np.float64)  # (tm is column-major)
    u, e, zero = np.linspace(-0.9, 0.9, 16), np.full(16, 1.0 - 1.2e-5), np.zeros(16)
    local = np.concatenate([np.stack(c, 1) for c in ((u, e, zero), (u, -e, zero), (e, u, zero), (-e, u, zero), (u, 0.5 * u[::-1], zero))])
    world = local @ tm.T + pos
    for what, d in (("down", (0.0, 0.0, -1.0)), ("oblique", (0.36, 0.48, -0.8)), ("from below", (0.0, 0.0, 1.0))):
        d = np.array(d)
        rays = make_rays(pkg, world - 50.0 * d, d.astype(np.float32))
        h = orc.trace_rays(scene, rays)
        q = (h["p"].astype(np.float64) - pos) @ np.linalg.inv(tm).T  # the hit points in the plane's own space
        zone = (h["node"] == 2) & (np.abs(q[:, :2]).max(axis=1) > 1.0 - 2e-5)
        print("plane edge zone, %s: %d of %d rays hit the plane, %d of them in the zone" % (what, int((h["node"] == 2).sum()), rays.size, int(zone.sum())))
        assert zone.sum() >= 40 and ((h["node"] == 2) & ~zone).sum() >= 8
        check_batch(pkg, orc, ctx, scene, rays, eye_of(scene), "plane edge zone, " + what)


# ---- family B --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(PROBES))
def test_b_probes(pkg, orc, ctx, golden, tag):
    scene = golden(tag).scene(pkg)
    ctx.upload(scene)
    for what, rays in family_b(pkg, tag):
        check_batch(pkg, orc, ctx, scene, rays, eye_of(scene), "B %s from %s" % (tag, what))


def test_b_probes_another_eye_and_other_depths(pkg, orc, ctx, golden):
    scene = golden("p4_240x135").scene(pkg)
    ctx.upload(scene)
    for what, rays in family_b(pkg, "p4_240x135"):
        check_batch(pkg, orc, ctx, scene, rays, (3.0, -30.0, 9.0), "B p4 from %s, eye (3, -30, 9)" % what)
        for k in (0, 2):
            check_batch(pkg, orc, ctx, scene, rays, eye_of(scene), "B p4 from %s, max_bounce %d" % (what, k), max_bounce=k)


# ---- family C --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(PROBES))
def test_c_tmax_at_the_hit(pkg, orc, ctx, golden, tag):
    scene = golden(tag).scene(pkg)
    ctx.upload(scene)
    fam = family_c(pkg, orc, scene, tag)
    assert len(fam) == (6 if tag in ("p4_240x135", "teapot2_240x135") else 4)
    for name, rays in fam:
        check_batch(pkg, orc, ctx, scene, rays, eye_of(scene), "C %s %s" % (tag, name))


# ---- family D --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(PROBES))
def test_d_rays_that_start_on_surfaces(pkg, orc, ctx, golden, tag):
    scene = golden(tag).scene(pkg)
    ctx.upload(scene)
    rays, _ = family_d(pkg, orc, scene, tag)
    check_batch(pkg, orc, ctx, scene, rays, eye_of(scene), "D %s" % tag)


# ---- family E --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["p4_240x135", "teapot2_240x135"])
def test_e_the_unit_length_band(pkg, orc, ctx, golden, tag):
    scene = golden(tag).scene(pkg)
    ctx.upload(scene)
    rays, ok, _ = family_e(pkg, tag)
    assert ok.sum() > 500 and (~ok).sum() > 500
    for ref in (False, True):
        h = ctx.trace_rays(rays, reference_walk=ref)
        flagged = (h["flags"] & pkg.RTU_RAY_INVALID) != 0
        print("E %s ref=%s: %d flagged invalid, %d by the binary32 rule, %d rays differ" % (tag, ref, int(flagged.sum()), int((~ok).sum()), int((flagged == ok).sum())))
        assert np.array_equal(flagged, ~ok)
        assert np.all(h["flags"][~ok] == pkg.RTU_RAY_INVALID)
    check_batch(pkg, orc, ctx, scene, rays, eye_of(scene), "E %s" % tag)
