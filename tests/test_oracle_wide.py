"""Scenes that are themselves wide — a thousand units and more across — and compact scenes whose node chain passes through a far-off
space, on the oracle alone: the families of tests/test_gpu_wide.py and what each must contain to test anything.

In both cases the rays that start at hit points (reflection, refraction, shadow rays) are far rays: Node::ToNodeCoords restates them
with a direction taken as (p + dir) - p in binary32 per level of the node's chain, and the line the reference tests leaves the ray's
own line by some 3 * 2^-24 * |p|^2 where it arrives. The fast variant bounds such rays by 1e-4 * max(scene scale, |origin|) alone
unless the scene is wide enough to need more (rtu_intersect.h, THE NEAR MARGIN).

  W1  a mirror wall at w = -c sends a render's reflection rays at a card at c = (X, 0.9 X, 0.3 X), both node orders, checkered
  W2  the same at a torus mesh, plain and under a rotated, non-uniformly scaled node, at X = 2000 and 4000 (at 1000 the near margin
      would skip 2 hits of 168 and none of 94; at 5000 the reference no longer sees the plain torus)
  W3  the same at a unit sphere, alone and with F2's card in front of its cube: a control for the S^2 / R widening of world_bounds,
      at X = 1000 and 2000 (at 5000 the reference's reflection rays no longer reach the sphere)
  W4  shadow rays across the scene: a floor patch around -c, a point light beyond c or a direct light along -c, the occluder's edge
      across the bundle of shadow rays, 10 units in front of the light (a), around c under a direct light (b) or 10 units above the
      floor (c: a control, the rays are short where they pass it)
  W5  a compact scene (world bounds 30) whose target sits in a group translated by G (1, 0.9, 0.3) and is translated back by the same,
      G = 0, 2e5 and 1e6 (at 2e4 a 128 x 128 frame holds 1 and 4 such hits, at 1e5 8 and 10)
  W6  W1 with a glass slab (two planes) in place of the mirror: refracted and internally reflected rays start at |p| ~ X

MODEL. `model_skips` of tests/test_oracle_far.py restates in binary64 the node-level test with the margin of a ray that starts in or
around the scene, 1e-4 * max(scene scale, |origin|): the margin every secondary and shadow ray had before a scene could ask for the
far term. The counts below are taken with it, on the oracle's own hits: they say that a family contains rays on which that margin
would lose a hit of the reference. What the device computes is compared with the oracle alone (tests/test_gpu_wide.py)."""
import math

import numpy as np
import pytest

from test_gpu_parity import _write_uv_mesh
from test_oracle_far import RTU_OBJ_PLANE, RTU_OBJ_SPHERE, RTU_OBJ_TRIMESH, impact_parameter, model_skips, model_world_bounds, node_of_type, to_object_space, torus
from test_oracle_rays import frame_of, make_rays, valid

SIZE = 128
S_CAM = 30.0
V = np.array([1.0, 0.9, 0.3])  # c = X * V, the far group of W5 is translated by G * V

MATERIALS = ('<material type="blinn" name="mirror"><diffuse r="0" g="0" b="0"/><specular value="0"/><reflection value="1"%s/></material>'
             '<material type="blinn" name="glass"><diffuse r="0" g="0" b="0"/><specular value="0"/><refraction index="1.5" value="0.9"/><reflection value="0.1"/></material>'
             '<material type="blinn" name="red"><diffuse r="0.9" g="0.2" b="0.1"/><specular value="0"/></material>'
             '<material type="blinn" name="grey"><diffuse r="0.7" g="0.7" b="0.7"/><specular value="0"/></material>'
             '<material type="blinn" name="checker"><diffuse r="1" g="1" b="1" texture="checkerboard"><color1 r="0.1" g="0.2" b="0.8"/>'
             '<color2 r="0.9" g="0.8" b="0.1"/><scale value="0.25"/></diffuse><specular value="0"/></material>')


def xyz(v):
    return 'x="%r" y="%r" z="%r"' % tuple(float(t) for t in v)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def facing(u):
    """XML of the rotation that takes +z to the unit vector u."""
    axis = np.cross([0.0, 0.0, 1.0], u)
    if np.linalg.norm(axis) < 1e-12:
        return "" if u[2] > 0 else '<rotate angle="180" x="1"/>'
    return '<rotate angle="%r" %s/>' % (math.degrees(math.acos(max(-1.0, min(1.0, float(u[2]))))), xyz(unit(axis)))


def turned_x(u):
    """Where the rotation of facing(u) takes +x (Rodrigues): the direction of an edge of a card that faces u."""
    k = np.cross([0.0, 0.0, 1.0], u)
    if np.linalg.norm(k) < 1e-12:
        return np.array([1.0, 0.0, 0.0])
    k, x = unit(k), np.array([1.0, 0.0, 0.0])
    cs, sn = float(u[2]), math.sqrt(max(0.0, 1.0 - float(u[2]) ** 2))
    return x * cs + np.cross(k, x) * sn + k * np.dot(k, x) * (1.0 - cs)


def camera_xml(pos, target, up, fov, size=SIZE):
    return ('<camera><position %s/><target %s/><up %s/><fov value="%r"/><width value="%d"/><height value="%d"/></camera>' %
            (xyz(pos), xyz(target), xyz(up), float(fov), size, size))


def load(pkg, tmp_path, name, objects, lights, camera, glossy=False):
    xml = tmp_path / (name + ".xml")
    xml.write_text("<xml><scene>%s%s%s</scene>%s</xml>" % ("".join(objects), MATERIALS % (' glossiness="0.05"' if glossy else ""), lights, camera))
    return pkg.Scene.from_xml(str(xml))


# ---- targets: XML of an object whose own transformation ends with a translation to `at` ----------------------------------------------
CARD_R, TORUS_R, SPHERE_R = 2.0, 2.7, 1.0
TILTED = '<scale x="1.5" y="0.7" z="2.0"/><rotate angle="40" x="0.3" y="1" z="0.2"/>'


def card(at, material="checker", turn='<rotate angle="90" x="1"/><rotate angle="-45" z="1"/>', name="card", scale=CARD_R):
    return '<object type="plane" name="%s" material="%s"><scale value="%r"/>%s<translate %s/></object>' % (name, material, float(scale), turn, xyz(at))


def mesh(tmp_path, at, xf=""):
    _write_uv_mesh(tmp_path / "torus.obj", 24, 10, torus)
    return '<object type="obj" name="%s/torus.obj" material="red">%s<translate %s/></object>' % (tmp_path, xf, xyz(at))


def ball(at):
    return '<object type="sphere" name="ball" material="red"><translate %s/></object>' % xyz(at)


def target_xml(tmp_path, what, at):
    """-> (XML, radius, type of the node whose hits are counted)"""
    if what in ("card", "plain card"):
        return card(at, "checker" if what == "card" else "red"), CARD_R, RTU_OBJ_PLANE
    if what == "torus":
        return mesh(tmp_path, at), TORUS_R, RTU_OBJ_TRIMESH
    if what == "tilted torus":
        return mesh(tmp_path, at, TILTED), 2.0 * TORUS_R, RTU_OBJ_TRIMESH
    assert what == "sphere"
    return ball(at), SPHERE_R, RTU_OBJ_SPHERE


def far_group(G, inner, levels=1):
    """`inner` (XML taking the translation of a target) inside a group translated by G * V and translated back by the same; levels = 3:
    three groups, the second undoes the first, the target undoes the third, which goes another way."""
    g = G * V
    if levels == 1:
        return '<object name="g"><translate %s/>%s</object>' % (xyz(g), inner(-g))
    assert levels == 3
    g3 = G * np.array([0.5, -1.0, 0.7])
    return ('<object name="g1"><translate %s/><object name="g2"><translate %s/><object name="g3"><translate %s/>%s</object></object></object>' %
            (xyz(g), xyz(-g), xyz(g3), inner(-g3)))


# ---- the mirror arrangement ----------------------------------------------------------------------------------------------------------
def mirror_camera(c, w, r, s=S_CAM):
    """The camera sees, in a wall through w with normal +z, the reflection of a target of radius r at c over a third of the image."""
    c, w = np.asarray(c, np.float64), np.asarray(w, np.float64)
    cm = np.array([c[0], c[1], 2.0 * w[2] - c[2]])
    E = w - s * unit(cm - w)
    fov = 2.0 * math.degrees(math.atan(6.0 * r / (s + np.linalg.norm(c - w))))
    return camera_xml(E, w, (0.0, 0.0, 1.0), fov)


def wide_lights(c):
    return ('<light type="ambient" name="a"><intensity value="0.3"/></light>'
            '<light type="direct" name="d"><intensity value="0.7"/><direction %s/></light>' % xyz(unit(c) * 0.8 + np.array([0.1, -0.2, -0.4])))


def soft_lights(c):
    """Recipes S and P: a point light of size 2 on the lit side of the target."""
    return ('<light type="ambient" name="a"><intensity value="0.3"/></light>'
            '<light type="point" name="p"><intensity value="0.7"/><position %s/><size value="2"/></light>' % xyz(np.asarray(c, np.float64) - 40.0 * unit(V) + np.array([5.0, -8.0, 12.0])))


def mirror_scene(pkg, tmp_path, what, X, wall_first=True, s=S_CAM, stochastic=False, G=None, levels=1, front_card=False, wall="mirror"):
    """W1-W3 (G is None): target `what` at c = X V, the wall at -c. W5 (G given): c = (10, 9, 3), w = -c, the target inside far_group(G).
    front_card (W3): F2's card 1.6 in front of the sphere's centre, across the reflected rays. wall = "glass": W6's slab, 0.5 thick."""
    c = X * V if G is None else 10.0 * V
    w = -c
    txml, r, _ = target_xml(tmp_path, what, c)
    if G is not None:
        txml = far_group(G, lambda off: target_xml(tmp_path, what, c + off)[0], levels)
    objs = [txml]
    if front_card:
        u = unit(w - c)
        objs.append(card(c + 1.6 * u, "grey", facing(u), name="front", scale=9.6))
    walls = ['<object type="plane" name="wall" material="%s"><scale value="20"/><translate %s/></object>' % (wall, xyz(w))]
    if wall == "glass":
        walls.append('<object type="plane" name="back" material="glass"><scale value="20"/><rotate angle="180" x="1"/><translate %s/></object>' % xyz(w - np.array([0.0, 0.0, 0.5])))
    objs = walls + objs if wall_first else objs[::-1] + walls
    return load(pkg, tmp_path, "wide", objs, soft_lights(c) if stochastic else wide_lights(c), mirror_camera(c, w, r, s), glossy=stochastic)


def wall_node(scene):
    """The wall is the only kind of node whose box is 40 units wide (a glass slab: its front, listed first)."""
    bounds, _ = model_world_bounds(scene)
    return [k for k in node_of_type(scene, RTU_OBJ_PLANE) if float((bounds[k][1] - bounds[k][0]).max()) > 30.0][0]


def nodes_named_first(scene):
    """Is the wall listed before the target?"""
    return wall_node(scene) == min(model_world_bounds(scene)[0])


def reflected(pkg, orc, scene, rays=None):
    """The reflection rays of a render, restated: the camera rays' closest hits on the wall (the oracle's p and N), the direction
    d - 2 (d . N) N in binary64, cast to binary32. They are caller rays that start where the render's own reflection rays start."""
    if rays is None:
        rays = pkg.camera_rays(frame_of(pkg, scene, SIZE, SIZE))
    assert valid(rays).all()
    h = orc.trace_rays(scene, rays, threads=8)
    on = h["node"] == wall_node(scene)
    d, N = rays["dir"][on].astype(np.float64), h["N"][on].astype(np.float64)
    out = make_rays(pkg, h["p"][on], unit_rows(d - 2.0 * (d * N).sum(axis=1)[:, None] * N))
    assert valid(out).all()
    return out


def unit_rows(a):
    return a / np.linalg.norm(a, axis=1)[:, None]


def skippable(orc, scene, rays, kind):
    """-> (hits of `rays` on the target nodes of type `kind`, how many of them the near margin's node test would skip, the hits)"""
    h = orc.trace_rays(scene, rays, threads=8)
    total = skipped = 0
    for k in node_of_type(scene, kind):
        if k == wall_node(scene):
            continue
        on = h["node"] == k
        total += int(on.sum())
        skipped += int((on & model_skips(scene, k, rays, h["t"].astype(np.float64))).sum())
    return total, skipped, h


W1 = [(X, first, what) for X in (100.0, 1000.0, 2000.0, 5000.0) for first in (True, False) for what in ("card",)] + [(1000.0, True, "plain card")]
W2 = [(X, what) for X in (2000.0, 4000.0) for what in ("torus", "tilted torus")]
W3 = [(X, front, first) for X in (1000.0, 2000.0) for front, first in ((False, True), (True, True), (True, False))]
W5_G = (0.0, 2e5, 1e6)
W5 = [(G, what, levels) for what in ("card", "torus") for G in W5_G for levels in (1,)] + [(W5_G[1], "card", 3)]
FLOOR = 10  # the least number of hits the near margin would lose, for a family to count as non-vacuous


@pytest.mark.parametrize("X,wall_first,what", W1)
def test_w1_mirror_to_card(pkg, orc, tmp_path, X, wall_first, what):
    scene = mirror_scene(pkg, tmp_path, what, X, wall_first)
    assert nodes_named_first(scene) == wall_first
    rays = reflected(pkg, orc, scene)
    total, skipped, _ = skippable(orc, scene, rays, RTU_OBJ_PLANE)
    print("W1 X=%g wall first=%s %s: %d reflection rays, %d hit the card, %d of those the near margin would skip" % (X, wall_first, what, rays.size, total, skipped))
    assert rays.size > SIZE * SIZE // 2 and total >= 50
    assert skipped == 0 if X == 100.0 else skipped >= FLOOR


@pytest.mark.parametrize("X,what", W2)
def test_w2_mirror_to_mesh(pkg, orc, tmp_path, X, what):
    scene = mirror_scene(pkg, tmp_path, what, X)
    rays = reflected(pkg, orc, scene)
    total, skipped, _ = skippable(orc, scene, rays, RTU_OBJ_TRIMESH)
    print("W2 X=%g %s: %d reflection rays, %d hit the mesh, %d of those the near margin would skip" % (X, what, rays.size, total, skipped))
    assert total >= 50 and skipped >= FLOOR


@pytest.mark.parametrize("X,front,wall_first", W3)
def test_w3_mirror_to_sphere_is_a_control(pkg, orc, tmp_path, X, front, wall_first):
    """world_bounds widens a sphere's box by 4e-6 S^2 / R, S the scene's diagonal: in a scene this wide that is more than the
    reference's line is off, and the near margin skips none of the sphere's hits although the sphere "grows" past its cube."""
    scene = mirror_scene(pkg, tmp_path, "sphere", X, wall_first, front_card=front)
    rays = reflected(pkg, orc, scene)
    k = node_of_type(scene, RTU_OBJ_SPHERE)[0]
    total, skipped, h = skippable(orc, scene, rays, RTU_OBJ_SPHERE)
    p, d = to_object_space(scene, k, rays)
    b = impact_parameter(p, d)[h["node"] == k]
    print("W3 X=%g front card=%s wall first=%s: %d reflection rays, %d hit the sphere (largest impact parameter %.3f), %d of those the near margin would skip" %
          (X, front, wall_first, rays.size, total, b.max() if b.size else 0.0, skipped))
    assert total >= (10 if front else 50) and skipped == 0
    if not front:
        assert b.max() > 1.3


@pytest.mark.parametrize("G,what,levels", W5)
def test_w5_compact_scene_far_chain(pkg, orc, tmp_path, G, what, levels):
    scene = mirror_scene(pkg, tmp_path, what, 10.0, G=G, levels=levels)
    _, scale = model_world_bounds(scene)
    rays = reflected(pkg, orc, scene)
    total, skipped, _ = skippable(orc, scene, rays, RTU_OBJ_PLANE if what == "card" else RTU_OBJ_TRIMESH)
    print("W5 G=%g %s levels=%d (largest |coordinate| of a bound %.1f): %d reflection rays, %d hit the target, %d of those the near margin would skip" %
          (G, what, levels, scale, rays.size, total, skipped))
    assert scale < 35.0 and total >= 50
    assert skipped == 0 if G == 0.0 else skipped >= FLOOR


def test_smallest_extents_with_a_skippable_hit(pkg, orc, tmp_path):
    """What the switch of near_margin (rtu_capi_build.hip; rtu_intersect.h, THE NEAR MARGIN) is held against: with nine times the rays
    (a 384 x 384 image) the smallest X at which the near margin would lose a hit of W1 is 250, the smallest G of W5 is 1e4; 20 000
    random rays from a wall patch once found 300 and 4000. The far term is on from X = 40 and G = 55: a quarter of the smallest of
    these is 62 and 1000."""
    dense = lambda scene: reflected(pkg, orc, scene, pkg.camera_rays(frame_of(pkg, scene, 3 * SIZE, 3 * SIZE)))
    found = {}
    for X in (62.0, 150.0, 200.0, 250.0, 300.0):
        scene = mirror_scene(pkg, tmp_path, "card", X)
        found["X=%g" % X] = skippable(orc, scene, dense(scene), RTU_OBJ_PLANE)[1]
    for G in (1e3, 4e3, 1e4, 2e4):
        for what, kind in (("card", RTU_OBJ_PLANE), ("torus", RTU_OBJ_TRIMESH)):
            scene = mirror_scene(pkg, tmp_path, what, 10.0, G=G)
            found["G=%g %s" % (G, what)] = skippable(orc, scene, dense(scene), kind)[1]
    print("hits the near margin would skip, of %d reflection rays: %s" % (9 * SIZE * SIZE, found))
    assert found["X=62"] == 0 and found["X=150"] == 0 and found["X=300"] > 0
    assert found["G=1000 card"] == 0 and found["G=1000 torus"] == 0 and found["G=20000 card"] + found["G=20000 torus"] > 0


def test_w6_glass_slab(pkg, orc, tmp_path):
    """A control for the counts: the slab's refracted rays are parallel to the camera's, i.e. aimed past the card's mirror image, so the
    card is seen by the slab's 10 % reflection alone — the same rays as W1's. What the family adds is on the device: rays that start
    inside the slab at |p| ~ X, refracted and internally reflected."""
    scene = mirror_scene(pkg, tmp_path, "card", 1000.0, wall="glass")
    rays = reflected(pkg, orc, scene)
    total, skipped, _ = skippable(orc, scene, rays, RTU_OBJ_PLANE)
    print("W6 X=1000: %d reflection rays off the slab's front, %d hit the card, %d of those the near margin would skip" % (rays.size, total, skipped))
    assert total >= 50 and skipped >= FLOOR


# ---- W4: shadows across the scene ----------------------------------------------------------------------------------------------------
def shadow_scene(pkg, tmp_path, what, X, variant, G=None):
    """A floor patch (a plane of half-width 20, normal +z) around f = -c seen from 30 units above. The occluder's centre is r off the
    central shadow ray, so that its edge crosses the bundle. variant "a": a point light at c + (0, 0, 50), the occluder 10 units in
    front of it as the floor sees it; "b": a direct light along -normalize(c), the occluder around c; "c": the point light again, the
    occluder 10 units from the floor. G: W5's compact scene, f = (-10, -9, -3), the light at (10, 9, 40), the occluder inside
    far_group(G). -> (scene, position of the light or None, unit vector towards a direct light or None)"""
    c = X * V if G is None else 10.0 * V
    f = -c
    L = c + np.array([0.0, 0.0, 50.0 if G is None else 37.0])
    u = unit(c - f) if variant == "b" else unit(L - f)
    # the card under the direct light and near the floor keeps W1's attitude, whose box is tight in z (its upper and lower edge);
    # every other occluder faces the rays, its edge (the card's, the torus's rim) r to the side
    upright = what == "card" and variant != "a"
    side = np.array([0.0, 0.0, 1.0]) if upright else turned_x(u)
    r = {"card": CARD_R, "torus": TORUS_R, "sphere": SPHERE_R}[what]
    # (a): the bundle is a few hundredths of a unit wide where it passes the occluder; it passes clear of the edge, by about half of
    # what the reference's line is off there, and the reference's noise alone decides which rays are occluded
    clear = 0.35 * (X / 1000.0) ** 2 if variant == "a" and G is None and what != "sphere" else 0.0
    centre = (c if variant == "b" else f + 10.0 * u if variant == "c" else L - 10.0 * u) + (r + clear) * side

    def occluder(at):
        if what == "card":
            return card(at, "red") if upright else card(at, "red", facing(u))
        return mesh(tmp_path, at, facing(u)) if what == "torus" else ball(at)
    oxml = occluder(centre) if G is None else far_group(G, lambda off: occluder(centre + off))
    floor = '<object type="plane" name="floor" material="grey"><scale value="20"/><translate %s/></object>' % xyz(f)
    light = ('<light type="direct" name="d"><intensity value="0.8"/><direction %s/></light>' % xyz(-u) if variant == "b" else
             '<light type="point" name="p"><intensity value="0.8"/><position %s/></light>' % xyz(L))
    # the shadow's edge on the floor is the occluder's, magnified by the ratio of the distances from the light
    half = 3.0 * r if variant != "c" else 3.0 * r * np.linalg.norm(L - f) / np.linalg.norm(L - centre)
    half = min(half, 12.0)
    cam = camera_xml(f + np.array([0.0, 0.0, 30.0]), f, (0.0, 1.0, 0.0), 2.0 * math.degrees(math.atan(half / 30.0)))
    scene = load(pkg, tmp_path, "shadow", [floor, oxml], '<light type="ambient" name="a"><intensity value="0.2"/></light>' + light, cam)
    return scene, (None if variant == "b" else L), (u if variant == "b" else None)


def shadow_rays(pkg, orc, scene, L, u):
    """The shadow rays of a render, restated: from the oracle's floor hits of the camera rays to the light, as caller rays."""
    rays = pkg.camera_rays(frame_of(pkg, scene, SIZE, SIZE))
    h = orc.trace_rays(scene, rays, threads=8)
    on = h["node"] == node_of_type(scene, RTU_OBJ_PLANE)[0]
    p = h["p"][on].astype(np.float64)
    if L is None:
        out = make_rays(pkg, p, np.broadcast_to(u, p.shape))
    else:
        out = make_rays(pkg, p, unit_rows(L - p), tmax=np.linalg.norm(L - p, axis=1).astype(np.float32))
    assert valid(out).all()
    return out


def occluder_node(scene, what):
    kind = {"card": RTU_OBJ_PLANE, "torus": RTU_OBJ_TRIMESH, "sphere": RTU_OBJ_SPHERE}[what]
    return node_of_type(scene, kind)[-1]  # (the floor is the first plane)


W4 = [(X, variant, what) for X in (1000.0, 5000.0) for variant in "abc" for what in ("card", "torus", "sphere")]
# the cases that hold at least FLOOR shadow rays which the reference finds occluded and the near margin's node test would let pass
W4_LIVE = {(1000.0, "b", "card"), (5000.0, "b", "card"), (5000.0, "b", "torus"), (5000.0, "a", "card"), (5000.0, "a", "torus")}


def shadow_counts(pkg, orc, scene, L, u, what):
    rays = shadow_rays(pkg, orc, scene, L, u)
    occ = orc.occluded_rays(scene, rays, threads=8) == 1
    return rays, occ, occ & model_skips(scene, occluder_node(scene, what), rays, rays["tmax"].astype(np.float64))


@pytest.mark.parametrize("X,variant,what", W4)
def test_w4_shadows_across_the_scene(pkg, orc, tmp_path, X, variant, what):
    """The rest are controls, and say why. Variant c: 10 units from its origin the reference's line is off by 1e-2 at most, a tenth
    of the near margin. The sphere: its widened box (W3); from X = 5000 under the direct light the reference no longer sees it at
    all. At X = 1000 the reference's line is off by 0.8 where it arrives: the torus's box and the box of a card that faces the rays are
    further than that from most of their rims, and only the upright card under the direct light has its edge ON its box."""
    scene, L, u = shadow_scene(pkg, tmp_path, what, X, variant)
    rays, occ, skipped = shadow_counts(pkg, orc, scene, L, u, what)
    print("W4%s X=%g %s: %d shadow rays, %d occluded, %d of those the near margin would let pass" % (variant, X, what, rays.size, int(occ.sum()), int(skipped.sum())))
    assert rays.size > SIZE * SIZE // 2 and occ.sum() <= rays.size - 50
    if (X, variant, what) in W4_LIVE:
        assert skipped.sum() >= FLOOR
    else:
        assert occ.sum() >= 10 or (X, variant, what) == (5000.0, "b", "sphere")
        assert skipped.sum() == 0


@pytest.mark.parametrize("G,what", [(G, what) for what in ("card", "torus") for G in W5_G])
def test_w5_shadows_through_a_far_chain(pkg, orc, tmp_path, G, what):
    """W4(a) in the compact scene, the light at (10, 9, 40). The shadow rays are 60 units long: the near margin loses occluded rays
    from G = 1e6 on; G = 2e5 is a control here (the mirror arrangement, whose rays graze the target's box, is live there)."""
    scene, L, u = shadow_scene(pkg, tmp_path, what, 10.0, "a", G=G)
    rays, occ, skipped = shadow_counts(pkg, orc, scene, L, u, what)
    print("W5 shadows G=%g %s: %d shadow rays, %d occluded, %d of those the near margin would let pass" % (G, what, rays.size, int(occ.sum()), int(skipped.sum())))
    assert 50 <= occ.sum() <= rays.size - 50
    if G >= 1e6:
        assert skipped.sum() >= FLOOR
    if G == 0.0:
        assert skipped.sum() == 0
