"""Renders and ray entries on rays whose origins lie far outside the scene, against the oracle: the families F1-F6 of
tests/test_oracle_far.py, which asserts on the oracle alone that each contains what it is meant to.

Renders (F1, F2, F4, F5): the counting variant equals the oracle (z bit for bit, colours within the project's bar, counters equal); the
fast variant with stage 2 cooperative and one lane per ray equals the counting variant bit for bit; so does the fast variant without
the node-level bounds (rtu_debug_node_bounds). F5 also as three frames in flight.
Ray entries (every family): rtu_trace_rays fast = reference walk = the oracle's ray-level entry, field by field by bits; the occlusion
byte likewise; rtu_shade_rays fast = reference walk by bytes, t equal to the oracle's by bits, colours within the bar, counters equal.

Every comparison of a test is made and printed before the first assertion, so that one run tells on how many rays each form fails."""
import numpy as np
import pytest

from test_gpu_parity import check_against
from test_gpu_ray_query import bits
from test_mesh_update_host import clone
from test_oracle_far import (F1, F2, F2_MESH, f2_mesh_scene, F5_CENTRE, F6_BACK, F6_VIEW, SIZE, f1_scene, f2_scene, f5_scene, f6_scene, family_f3, family_f6,
                             plane_scene, teapot_scene, torus_scene)
from test_oracle_rays import frame_of, valid

pytestmark = pytest.mark.gpu

FIELDS = ("t", "flags", "node", "material", "p", "N")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def differing(a, b):
    """Number of rows (pixels, rays) of two arrays of 32-bit items that differ in some bit."""
    d = bits(a) != bits(b)
    return int(d.reshape(d.shape[0], -1).any(axis=1).sum()) if d.ndim > 1 else int(d.sum())


def hits_differing(a, b):
    bad = np.zeros(a.size, bool)
    for f in FIELDS:
        d = bits(a[f]) != bits(b[f])
        bad |= d.any(axis=1) if d.ndim > 1 else d
    return int(bad.sum())


def fast_figures(pkg, ctx, fig, cnt, make_frame, flags=(0,)):
    """Adds to `fig`, per combination of node-level bounds on / off, stage 2 per ray / cooperative and rtu_debug_flags in `flags`
    (64: the occluder lists only say "empty cell or not"), the number of pixels at which the fast variant differs from `cnt`."""
    try:
        for on in (1, 0):
            assert pkg.hip.rtu_debug_node_bounds(ctx._h, on) == 0
            for thr in (1, 10 ** 9):
                for dbg in flags:
                    assert pkg.hip.rtu_debug_flags(ctx._h, dbg) == 0
                    fr = make_frame()
                    fr.coop_threshold = thr
                    fast = ctx.render(fr)[0]
                    name = "fast (bounds %d, coop_threshold %d%s) != counting" % (on, thr, ", flags %d" % dbg if dbg else "")
                    fig[name] = differing(fast.reshape(-1, 4), cnt.reshape(-1, 4))
    finally:
        pkg.hip.rtu_debug_node_bounds(ctx._h, 1)
        pkg.hip.rtu_debug_flags(ctx._h, 0)


def render_figures(pkg, orc, ctx, scene, w, h, label, flags=(0,)):
    """The scene is uploaded. Returns (figures: name -> number of differing pixels or 0 / 1, the counting image, the oracle's)."""
    cam = scene.desc.camera
    cpu, cst = orc.render(scene, w, h, threads=8)
    cnt, gst = ctx.render(pkg.frame_setup(cam, w, h, collect_stats=True), stats=True)
    fig = {"counting z != oracle": differing(cnt[..., 3].reshape(-1), cpu[..., 3].reshape(-1)), "counters != oracle": int(gst != cst)}
    fast_figures(pkg, ctx, fig, cnt, lambda: pkg.frame_setup(cam, w, h), flags)
    print("%s render %dx%d, %d hit pixels: %s" % (label, w, h, int((cpu[..., 3] != np.float32(1e30)).sum()), fig))
    return fig, cnt, cpu


def sampled_figures(pkg, orc, ctx, scene, size, spp, gather, label, flags=(0,)):
    """The scene is uploaded. A frame of recipe S (gather 0) or P on the keyed sample streams: (figures, the counting image, the oracle's)."""
    cam = scene.desc.camera
    cpu, cst = (orc.render_paths if gather else orc.render_samples)(scene, size, size, spp, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=8)
    cnt, gst = ctx.render(pkg.frame_setup(cam, size, size, collect_stats=True, samples=spp, gather_bounces=gather), stats=True)
    fig = {"counting z != oracle": differing(cnt[..., 3].reshape(-1), cpu[..., 3].reshape(-1)), "counters != oracle": int(gst != cst)}
    fast_figures(pkg, ctx, fig, cnt, lambda: pkg.frame_setup(cam, size, size, samples=spp, gather_bounces=gather), flags)
    print("%s: %s" % (label, fig))
    return fig, cnt, cpu


def settle_sampled(orc, fig, cnt, cpu, gather):
    """The bars of the sampled frames: recipe S within 3e-4 (tests/test_gpu_fuzz.py: the sum over samples); recipe P 8-bit +-1 and
    linear RGB to 1e-3 of max(value, 1e-2) (tests/test_gpu_sampled.py: the chain multiplies up to five Shade() trees)."""
    if not gather:
        settle(orc, [fig], [(cnt, cpu)], rel_tol=3e-4)
        return
    settle(orc, [fig], [])
    d8 = np.abs(orc.postprocess(cnt)[0].astype(np.int32) - orc.postprocess(cpu)[0].astype(np.int32))
    assert d8.max() <= 1, "8-bit RGB differs by %d levels at %d pixels" % (d8.max(), (d8 > 1).sum())
    d = np.abs(cnt[..., :3].astype(np.float64) - cpu[..., :3].astype(np.float64))
    assert (d / np.maximum(np.abs(cpu[..., :3]), 1e-2)).max() < 1e-3


def ray_figures(pkg, orc, ctx, scene, rays, eye, label):
    """The scene is uploaded. Returns (figures, the fast radiance, the oracle's radiance)."""
    assert valid(rays).all() and rays.size > 0
    want = orc.trace_rays(scene, rays, threads=8)
    fast, ref = ctx.trace_rays(rays), ctx.trace_rays(rays, reference_walk=True)
    occ = orc.occluded_rays(scene, rays, threads=8)
    cpu, cst = orc.shade_rays(scene, rays, eye, threads=8)
    out = ctx.shade_rays(rays, eye)[0]
    sref, gst = ctx.shade_rays(rays, eye, reference_walk=True, stats=True)
    fig = {"trace fast != oracle": hits_differing(fast, want), "trace reference walk != oracle": hits_differing(ref, want),
           "occluded fast != oracle": int((ctx.occluded(rays) != occ).sum()),
           "occluded reference walk != oracle": int((ctx.occluded(rays, reference_walk=True) != occ).sum()),
           "shade fast != reference walk": differing(out, sref), "shade reference walk t != oracle": differing(sref[:, 3], cpu[:, 3]),
           "shade counters != oracle": int(gst != cst)}
    print("%s: %d rays, %d hits, %d occluded: %s" % (label, rays.size, int(((want["flags"] & orc.RAY_HIT) != 0).sum()), int(occ.sum()), fig))
    return fig, out, cpu


def settle(orc, figs, images, rel_tol=None):
    """After every figure is printed: all of them zero, and each (device image, oracle image) pair within the colour bar."""
    bad = {k: v for fig in figs for k, v in fig.items() if v}
    assert not bad, "differences: %s" % bad
    for dev, cpu in images:
        if rel_tol is None:
            check_against(dev, cpu, orc)
        else:
            check_against(dev, cpu, orc, rel_tol=rel_tol)


def render_and_rays(pkg, orc, ctx, scene, w, h, label, rel_tol=None):
    ctx.upload(scene)
    frame = frame_of(pkg, scene, w, h)
    rays = pkg.camera_rays(frame)
    rfig, cnt, cpu = render_figures(pkg, orc, ctx, scene, w, h, label)
    qfig, out, qcpu = ray_figures(pkg, orc, ctx, scene, rays, tuple(frame.cam_pos), label + " camera rays")
    # the entry and the render answer the same rays
    rfig["shade_rays != the render"] = differing(out, cnt.reshape(-1, 4))
    print("%s: shade_rays differs from the render at %d pixels" % (label, rfig["shade_rays != the render"]))
    settle(orc, [rfig, qfig], [(cnt, cpu), (out.reshape(1, -1, 4), qcpu.reshape(1, -1, 4))], rel_tol)
    return rays


# ---- F1 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(F1))
def test_f1_lone_sphere(pkg, orc, ctx, tmp_path, name):
    render_and_rays(pkg, orc, ctx, f1_scene(pkg, tmp_path, name), SIZE, SIZE, "F1 " + name)


# ---- F2 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,zc,card_first", F2)
def test_f2_sphere_and_card(pkg, orc, ctx, tmp_path, D, zc, card_first):
    render_and_rays(pkg, orc, ctx, f2_scene(pkg, tmp_path, D, zc, card_first), SIZE, SIZE, "F2 D=%g zc=%g card first=%s" % (D, zc, card_first))


@pytest.mark.parametrize("D,zc,card_first", F2_MESH)
def test_f2_with_a_mesh_stage_2_of_the_primary_rays(pkg, orc, ctx, tmp_path, D, zc, card_first):
    """A torus around the sphere: the pixels on which the node-level test could go wrong enter the torus's box, are deferred, and are
    traced again by the stage-2 kernels (cooperative at coop_threshold 10**9, one lane per ray at 1), which bound the ray per ray."""
    render_and_rays(pkg, orc, ctx, f2_mesh_scene(pkg, tmp_path, D, zc, card_first), SIZE, SIZE, "F2 + torus D=%g zc=%g card first=%s" % (D, zc, card_first))


SAMPLED = [(D, zc, first, mesh, 0) for D, zc, first in F2_MESH for mesh in (False, True)] + [F2_MESH[0] + (True, 4)]  # the last: recipe P


@pytest.mark.parametrize("D,zc,card_first,mesh,gather", SAMPLED)
def test_f2_sampled_frames_from_afar(pkg, orc, ctx, tmp_path, D, zc, card_first, mesh, gather):
    """Recipe S (two samples per pixel): its primary rays have no node rectangle and are bounded per ray, in stage 1 and, with the
    torus, in stage 2. Against the oracle on the keyed sample streams: z bit for bit, colours within the bar of the sampled random
    scenes (tests/test_gpu_fuzz.py: 3e-4, the sum over samples), counters equal; the fast variant with both stage-2 forms and
    without the node-level bounds equals the counting variant bit for bit. One frame of recipe P (gather 4: the same primary walk, plus
    the gather chain, whose rays start at hit points): its colour bar is that of tests/test_gpu_sampled.py, 8-bit +-1 and linear RGB
    to 1e-3 of max(value, 1e-2) — the chain multiplies up to five Shade() trees."""
    scene = (f2_mesh_scene if mesh else f2_scene)(pkg, tmp_path, D, zc, card_first)
    ctx.upload(scene)
    fig, cnt, cpu = sampled_figures(pkg, orc, ctx, scene, SIZE, 2, gather, "F2 sampled D=%g zc=%g card first=%s torus=%s gather=%d" % (D, zc, card_first, mesh, gather))
    settle_sampled(orc, fig, cnt, cpu, gather)


# ---- F3 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["unit D=5e3", "R=0.05 D/R=5e3"])
def test_f3_rays_that_end_in_front_of_the_box(pkg, orc, ctx, tmp_path, name):
    scene = f1_scene(pkg, tmp_path, name)
    ctx.upload(scene)
    frame = frame_of(pkg, scene, SIZE, SIZE)
    short = family_f3(pkg, orc, scene, pkg.camera_rays(frame))
    assert short.size >= 50
    fig, out, cpu = ray_figures(pkg, orc, ctx, scene, short, tuple(frame.cam_pos), "F3 " + name)
    settle(orc, [fig], [(out.reshape(1, -1, 4), cpu.reshape(1, -1, 4))])


# ---- F4 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1e3, 5e3])
@pytest.mark.parametrize("what", ["torus", "teapot", "plane"])
def test_f4_controls(pkg, orc, ctx, golden, tmp_path, what, D):
    if what == "teapot":
        scene = teapot_scene(pkg, golden, D)
        w, h = scene.desc.camera.img_width, scene.desc.camera.img_height
    else:
        scene = torus_scene(pkg, tmp_path, D) if what == "torus" else plane_scene(pkg, tmp_path, D)
        w = h = SIZE
    render_and_rays(pkg, orc, ctx, scene, w, h, "F4 %s D=%g" % (what, D))


# ---- F5 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [100.0, 1000.0])
@pytest.mark.parametrize("tag", sorted(F5_CENTRE))
def test_f5_golden_scenes_from_afar(pkg, orc, ctx, golden, tag, factor):
    g = golden(tag)
    scene = f5_scene(pkg, golden, tag, factor)
    W, H = g.width, g.height
    render_and_rays(pkg, orc, ctx, scene, W, H, "F5 %s x%g" % (tag, factor))
    # three frames in flight: the far camera, and two with a wider field of view
    cams = []
    for i in range(3):
        cam = type(scene.desc.camera).from_buffer_copy(scene.desc.camera)
        cam.fov *= 1.0 + 0.25 * i
        cams.append(cam)
    singles = [ctx.render(pkg.frame_setup(c, W, H))[0] for c in cams]
    d = pkg.hip.rtu_device_alloc(ctx._h, 3 * W * H * 16)
    try:
        ctx.render_frames_device([pkg.frame_setup(c, W, H) for c in cams], d)
        ctx.frame_status()
        got = np.empty((3, H, W, 4), np.float32)
        assert pkg.hip.rtu_copy_to_host(ctx._h, got.ctypes.data, d, got.nbytes) == 0
    finally:
        pkg.hip.rtu_device_free(ctx._h, d)
    bad = [differing(got[i].reshape(-1, 4), singles[i].reshape(-1, 4)) for i in range(3)]
    print("F5 %s x%g: frames in flight differ from single frames at %s pixels" % (tag, factor, bad))
    assert not any(bad)
    for i in (1, 2):  # the wider frames against the oracle too
        other = clone(pkg, scene)
        other.desc.camera.fov = cams[i].fov
        check_against(got[i], orc.render(other, W, H, threads=8)[0], orc)


# ---- F6 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("back", F6_BACK)
@pytest.mark.parametrize("name", sorted(F6_VIEW))
def test_f6_grids_from_beyond_a_cameras_reach(pkg, orc, ctx, golden, name, back):
    scene = f6_scene(pkg, golden, name)
    ctx.upload(scene)
    eye = tuple(float(x) for x in scene.desc.camera.pos)
    figs, images = [], []
    for what, rays in family_f6(pkg, name, back):
        fig, out, cpu = ray_figures(pkg, orc, ctx, scene, rays, eye, "F6 %s back=%g %s" % (name, back, what))
        figs.append({"%s: %s" % (what, k): v for k, v in fig.items()})
        images.append((out.reshape(1, -1, 4), cpu.reshape(1, -1, 4)))
    settle(orc, figs, images)
