"""Renders and ray entries on wide scenes and on compact scenes with a far node chain, against the oracle: the families W1-W6 of
tests/test_oracle_wide.py, which asserts on the oracle alone that each contains rays on which the margin of a ray "that starts in or
around the scene" would lose a hit of the reference.

Per scene: the counting variant equals the oracle (z bit for bit, colours within the project's bar, counters equal); the fast variant
equals the counting variant bit for bit with stage 2 cooperative and one lane per ray, with and without the node-level bounds
(rtu_debug_node_bounds), with the occluder lists whole and reduced to "empty cell or not" (rtu_debug_flags 64) — each combination
its own figure, so that one run tells which mechanism loses how many pixels. The camera rays through rtu_shade_rays: fast = reference
walk by bytes, t equal to the oracle's by bits, equal to the render at every pixel. And the render's own reflection or shadow rays,
restated as caller rays (which every walk bounds by the far margin), through rtu_trace_rays / rtu_occluded_rays / rtu_shade_rays.

Every figure of a test is printed before the first assertion."""
import ctypes

import numpy as np
import pytest

from test_gpu_far import differing, ray_figures, render_figures, sampled_figures, settle, settle_sampled
from test_gpu_parity import check_against
from test_gpu_ray_query import nodes
from test_mesh_update_host import clone
from test_oracle_rays import frame_of
from test_oracle_wide import SIZE, W1, W2, W3, W4, W5, W5_G, mirror_scene, reflected, shadow_rays, shadow_scene

pytestmark = pytest.mark.gpu

FLAGS = (0, 64)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def wide_figures(pkg, orc, ctx, scene, label, restate):
    """Uploads the scene; the render, its camera rays and the rays `restate(camera rays)` gives; then every assertion."""
    ctx.upload(scene)
    frame = frame_of(pkg, scene, SIZE, SIZE)
    eye = tuple(frame.cam_pos)
    rays = pkg.camera_rays(frame)
    rfig, cnt, cpu = render_figures(pkg, orc, ctx, scene, SIZE, SIZE, label, flags=FLAGS)
    qfig, out, qcpu = ray_figures(pkg, orc, ctx, scene, rays, eye, label + " camera rays")
    rfig["shade_rays != the render"] = differing(out, cnt.reshape(-1, 4))
    print("%s: shade_rays differs from the render at %d pixels" % (label, rfig["shade_rays != the render"]))
    again = restate(rays)
    sfig, sout, scpu = ray_figures(pkg, orc, ctx, scene, again, eye, label + " restated rays")
    sfig = {"restated: " + k: v for k, v in sfig.items()}
    settle(orc, [rfig, qfig, sfig], [(cnt, cpu), (out.reshape(1, -1, 4), qcpu.reshape(1, -1, 4)), (sout.reshape(1, -1, 4), scpu.reshape(1, -1, 4))])


def mirror_figures(pkg, orc, ctx, scene, label):
    wide_figures(pkg, orc, ctx, scene, label, lambda rays: reflected(pkg, orc, scene, rays))


@pytest.mark.parametrize("X,wall_first,what", W1 + [(2e4, True, "card")])
def test_w1_mirror_to_card(pkg, orc, ctx, tmp_path, X, wall_first, what):
    """X = 2e4 is beyond the reach of binary32: the reference's reflection rays hit nothing any more, and neither do the device's."""
    scene = mirror_scene(pkg, tmp_path, what, X, wall_first)
    if X >= 2e4:
        hit = orc.trace_rays(scene, reflected(pkg, orc, scene), threads=8)
        assert not ((hit["flags"] & orc.RAY_HIT) != 0).any()
    mirror_figures(pkg, orc, ctx, scene, "W1 X=%g wall first=%s %s" % (X, wall_first, what))


@pytest.mark.parametrize("X,what", W2)
def test_w2_mirror_to_mesh(pkg, orc, ctx, tmp_path, X, what):
    mirror_figures(pkg, orc, ctx, mirror_scene(pkg, tmp_path, what, X), "W2 X=%g %s" % (X, what))


@pytest.mark.parametrize("X,front,wall_first", W3)
def test_w3_mirror_to_sphere(pkg, orc, ctx, tmp_path, X, front, wall_first):
    mirror_figures(pkg, orc, ctx, mirror_scene(pkg, tmp_path, "sphere", X, wall_first, front_card=front), "W3 X=%g front card=%s wall first=%s" % (X, front, wall_first))


@pytest.mark.parametrize("G,what,levels", W5)
def test_w5_compact_scene_far_chain(pkg, orc, ctx, tmp_path, G, what, levels):
    mirror_figures(pkg, orc, ctx, mirror_scene(pkg, tmp_path, what, 10.0, G=G, levels=levels), "W5 G=%g %s levels=%d" % (G, what, levels))


def test_w6_glass_slab(pkg, orc, ctx, tmp_path):
    mirror_figures(pkg, orc, ctx, mirror_scene(pkg, tmp_path, "card", 1000.0, wall="glass"), "W6 X=1000")


@pytest.mark.parametrize("X,variant,what", W4)
def test_w4_shadows_across_the_scene(pkg, orc, ctx, tmp_path, X, variant, what):
    scene, L, u = shadow_scene(pkg, tmp_path, what, X, variant)
    wide_figures(pkg, orc, ctx, scene, "W4%s X=%g %s" % (variant, X, what), lambda rays: shadow_rays(pkg, orc, scene, L, u))


@pytest.mark.parametrize("G,what", [(G, what) for what in ("card", "torus") for G in W5_G])
def test_w5_shadows_through_a_far_chain(pkg, orc, ctx, tmp_path, G, what):
    scene, L, u = shadow_scene(pkg, tmp_path, what, 10.0, "a", G=G)
    wide_figures(pkg, orc, ctx, scene, "W5 shadows G=%g %s" % (G, what), lambda rays: shadow_rays(pkg, orc, scene, L, u))


# ---- sampled frames ----------------------------------------------------------------------------------------------------------------
def sampled_scene(pkg, tmp_path, which):
    """One W1 and one W5 scene made stochastic: the mirror glossy (0.05), a point light of size 2."""
    return mirror_scene(pkg, tmp_path, "card", 1000.0, stochastic=True) if which == "W1" else mirror_scene(pkg, tmp_path, "card", 10.0, G=W5_G[1], stochastic=True)


@pytest.mark.parametrize("gather", [0, 4])
@pytest.mark.parametrize("which", ["W1", "W5"])
def test_sampled_frames(pkg, orc, ctx, tmp_path, which, gather):
    """Recipe S (two samples per pixel) and recipe P (the same with gather_bounces 4) on the keyed sample streams with portable
    trigonometry, with the bars of test_f2_sampled_frames_from_afar; the fast variant equals the counting variant bit for bit."""
    scene = sampled_scene(pkg, tmp_path, which)
    ctx.upload(scene)
    fig, cnt, cpu = sampled_figures(pkg, orc, ctx, scene, SIZE, 2, gather, "%s sampled gather=%d" % (which, gather), flags=FLAGS)
    settle_sampled(orc, fig, cnt, cpu, gather)


# ---- three frames in flight --------------------------------------------------------------------------------------------------------
def test_three_frames_in_flight(pkg, orc, ctx, tmp_path):
    """One W1 scene, the camera at three distances s from the wall: the frames in flight equal the single frames bit for bit, and the
    oracle's within the bar."""
    scenes = [mirror_scene(pkg, tmp_path, "card", 1000.0, s=s) for s in (20.0, 30.0, 45.0)]
    ctx.upload(scenes[1])
    cams = [type(sc.desc.camera).from_buffer_copy(sc.desc.camera) for sc in scenes]
    singles = [ctx.render(pkg.frame_setup(c, SIZE, SIZE))[0] for c in cams]
    d = pkg.hip.rtu_device_alloc(ctx._h, 3 * SIZE * SIZE * 16)
    try:
        ctx.render_frames_device([pkg.frame_setup(c, SIZE, SIZE) for c in cams], d)
        ctx.frame_status()
        got = np.empty((3, SIZE, SIZE, 4), np.float32)
        assert pkg.hip.rtu_copy_to_host(ctx._h, got.ctypes.data, d, got.nbytes) == 0
    finally:
        pkg.hip.rtu_device_free(ctx._h, d)
    cpus = [orc.render(sc, SIZE, SIZE, threads=8)[0] for sc in scenes]
    bad = [differing(got[i].reshape(-1, 4), singles[i].reshape(-1, 4)) for i in range(3)]
    badz = [differing(got[i][..., 3].reshape(-1), cpus[i][..., 3].reshape(-1)) for i in range(3)]
    print("W1 X=1000: frames in flight differ from single frames at %s pixels, their z from the oracle's at %s" % (bad, badz))
    assert not any(bad) and not any(badz)
    for i in range(3):
        check_against(got[i], cpus[i], orc)


# ---- a scene update ----------------------------------------------------------------------------------------------------------------
def moved_to(pkg, scene, other):
    """A copy of `scene` with every node and the camera where `other` (the same scene at another size) has them."""
    out = clone(pkg, scene)
    assert out.desc.n_nodes == other.desc.n_nodes
    for i in range(out.desc.n_nodes):
        assert nodes(out)[i].obj_type == nodes(other)[i].obj_type
        for f in ("tm", "itm", "pos"):
            for k in range(len(getattr(nodes(out)[i], f))):
                getattr(nodes(out)[i], f)[k] = getattr(nodes(other)[i], f)[k]
    ctypes.memmove(ctypes.addressof(out.desc.camera), ctypes.addressof(other.desc.camera), ctypes.sizeof(other.desc.camera))
    return out


@pytest.mark.parametrize("X0,X1", [(100.0, 5000.0), (5000.0, 100.0)])
@pytest.mark.parametrize("what", ["card", "torus"])
def test_scene_update_between_compact_and_wide(pkg, orc, tmp_path, what, X0, X1):
    """W1 (and the torus of W2) uploaded at one size, then moved by rtu_update_scene to the other, the camera following: the images
    equal a fresh upload's bit for bit (the margins' constants, the node bounds and the occluder lists follow the update), the
    fast variant equals the counting variant, and the counting variant the oracle."""
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    first = mirror_scene(pkg, tmp_path / "a", what, X0)
    moved = moved_to(pkg, first, mirror_scene(pkg, tmp_path / "b", what, X1))
    old, new = pkg.Context(0), pkg.Context(0)
    try:
        old.upload(first)
        old.render(frame_of(pkg, first, SIZE, SIZE))
        old.update(moved)
        new.upload(moved)
        fig_old, cnt_old, cpu = render_figures(pkg, orc, old, moved, SIZE, SIZE, "%s X=%g updated to X=%g" % (what, X0, X1), flags=FLAGS)
        fig_new, cnt_new, _ = render_figures(pkg, orc, new, moved, SIZE, SIZE, "%s X=%g uploaded" % (what, X1), flags=FLAGS)
        fast_old, fast_new = old.render(frame_of(pkg, moved, SIZE, SIZE))[0], new.render(frame_of(pkg, moved, SIZE, SIZE))[0]
        fig = {"updated counting != uploaded counting": differing(cnt_old.reshape(-1, 4), cnt_new.reshape(-1, 4)),
               "updated fast != uploaded fast": differing(fast_old.reshape(-1, 4), fast_new.reshape(-1, 4))}
        print("%s X=%g -> %g: %s" % (what, X0, X1, fig))
        settle(orc, [{"updated: " + k: v for k, v in fig_old.items()}, {"uploaded: " + k: v for k, v in fig_new.items()}, fig], [(cnt_old, cpu), (cnt_new, cpu)])
    finally:
        old.close()
        new.close()
