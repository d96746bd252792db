"""The shading arithmetic at the inputs where a scene constant or an already computed value can stand in for a per-pixel
normalisation: the normal of a plane hit (a constant of the node's chain and the side hit), the direction of a direct light (a constant
of the light), a point light's direction (the negative of its shadow ray's), the view vector of a material without a highlight.

The first of these is in the kernels: the fast variant reads a plane hit's world normal from DevNode::plane_n (rtu_intersect.h trace;
rtu_debug_flags 4096 switches it off). The others were built and measured and did not pay (NOTEBOOK.md, "Shading with fewer
normalisations"); their cases stay as the statement of what any such shortcut has to reproduce, and as parity tests of inputs no
golden scene has — non-finite chains, light vectors that normalise to infinities, zeros or NaN, a light or the eye at a hit point.
Every case asserts three things on an image of 64 x 48: the fast variant equals the counting variant (which keeps the literal
arithmetic) as uint32, it equals itself with rtu_debug_flags 4096, and it equals the oracle: z bit for bit, colours as
test_gpu_parity.check_against compares them (NaN colours at the same pixels)."""
import ctypes

import numpy as np
import pytest

from test_gpu_parity import check_against, ctx  # noqa: F401  (ctx: the module-scoped context fixture)
from test_light_lists import RtuLight

pytestmark = pytest.mark.gpu

LITERAL = 4096  # rtu_debug_flags: plane normals through the chain's transformations, not from the node's table
W, H = 64, 48

MATERIALS = """
  <material type="blinn" name="matte"><diffuse r="0.8" g="0.7" b="0.6"/><specular value="0"/></material>
  <material type="blinn" name="shiny"><diffuse r="0.3" g="0.5" b="0.7"/><specular value="0.8"/><glossiness value="20"/></material>
  <material type="blinn" name="mirror"><diffuse r="0.4" g="0.4" b="0.4"/><specular value="0.5"/><glossiness value="40"/><reflection value="0.5"/></material>
"""


def camera(pos, target, up=(0, 0, 1), fov=50):
    return ('<camera><position x="%r" y="%r" z="%r"/><target x="%r" y="%r" z="%r"/><up x="%r" y="%r" z="%r"/><fov value="%r"/>'
            '<width value="%d"/><height value="%d"/></camera>' % (tuple(pos) + tuple(target) + tuple(up) + (fov, W, H)))


def load(pkg, tmp_path, objects, lights, cam, name="s.xml"):
    xml = tmp_path / name
    xml.write_text("<xml><scene>%s%s%s</scene>%s</xml>" % (objects, MATERIALS, lights, cam))
    return pkg.Scene.from_xml(str(xml))


def lights_of(scene):
    return ctypes.cast(scene.desc.lights, ctypes.POINTER(RtuLight))


def set_light_vec(scene, index, vec, intensity=None):
    nl = RtuLight.from_buffer_copy(bytes(lights_of(scene)[index]))
    nl.vec[0], nl.vec[1], nl.vec[2] = [float(v) for v in vec]
    if intensity is not None:
        nl.intensity[0] = nl.intensity[1] = nl.intensity[2] = float(intensity)
    scene.set_light(index, nl)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def render(pkg, ctx, scene, stats):
    fr = pkg.frame_setup(scene.desc.camera, W, H, collect_stats=stats)
    return ctx.render(fr, stats=stats)[0]


def both_ways(pkg, orc, ctx, scene, upload=True):
    """The three assertions of every case on the scene the context holds (or uploads); returns the fast variant's image."""
    if upload:
        ctx.upload(scene)
    fast = render(pkg, ctx, scene, False)
    counting = render(pkg, ctx, scene, True)
    try:
        assert pkg.hip.rtu_debug_flags(ctx._h, LITERAL) == 0
        literal = render(pkg, ctx, scene, False)
    finally:
        pkg.hip.rtu_debug_flags(ctx._h, 0)
    assert np.array_equal(bits(fast), bits(counting)), "fast and counting variants differ at %d values" % int((bits(fast) != bits(counting)).sum())
    assert np.array_equal(bits(fast), bits(literal)), "the fast variant differs with debug flag 4096 at %d values" % int((bits(fast) != bits(literal)).sum())
    cpu, _ = orc.render(scene, W, H, threads=4)
    check_against(fast, cpu, orc)
    return fast


def hit_points(pkg, orc, scene):
    """Per pixel, Trace() of the primary ray by the oracle: the structured hits [H, W] (p as the renders compute it, bit for bit)."""
    fr = pkg.frame_setup(scene.desc.camera, W, H)
    return orc.trace_rays(scene, pkg.camera_rays(fr), threads=4).reshape(H, W)


TWO_LIGHTS = """
  <light type="ambient" name="amb"><intensity value="0.1"/></light>
  <light type="point" name="pt"><intensity value="0.7"/><position x="3" y="-4" z="9"/></light>
  <light type="direct" name="dir"><intensity value="0.5"/><direction x="-0.3" y="0.4" z="-1"/></light>
"""

# ---- B: plane normals per node -----------------------------------------------------------------------------------------

NESTED = """
  <object name="g1"><rotate angle="20" x="1" y="0.2" z="0.1"/><scale x="1.3" y="0.8" z="1.1"/><translate x="0.5" y="1" z="0.2"/>
    <object name="g2"><scale x="0.9" y="1.4" z="0.7"/><rotate angle="-35" z="1"/><translate x="-1" z="0.5"/>
      <object type="plane" name="up" material="%s"><scale x="4" y="3" z="1"/><rotate angle="10" y="1"/><translate x="-3.5" z="-1"/></object>
      <object type="plane" name="down" material="%s"><scale x="4" y="3" z="1"/><rotate angle="170" y="1"/><translate x="4" z="1"/></object>
    </object></object>
  <object type="sphere" name="ball" material="shiny"><scale value="0.8"/><translate x="0" y="0" z="1.5"/></object>
"""
OTHER_CHAIN = """
  <object name="h"><rotate angle="-15" y="1"/><scale x="2" y="1" z="0.5"/>
    <object type="plane" name="third" material="matte"><scale value="20"/><rotate angle="5" x="1"/><translate z="-3"/></object></object>
"""
CAM_ABOVE = camera((1, -14, 7), (0, 0, 0))


def test_plane_front_and_back_under_nested_parents(pkg, orc, ctx, tmp_path):
    """Two planes under two nested parents with rotations and non-uniform scales: the camera sees the front of one and the back of
    the other (a mirror, so the back side's normal reaches pixels too), and a third plane with another chain behind them."""
    scene = load(pkg, tmp_path, NESTED % ("mirror", "mirror") + OTHER_CHAIN, TWO_LIGHTS, CAM_ABOVE)
    hits = hit_points(pkg, orc, scene)
    seen = {int(n): sorted(set((hits["flags"][hits["node"] == n] & 3).tolist())) for n in np.unique(hits["node"]) if n >= 0}
    assert len(seen) >= 4 and [1] in seen.values() and [3] in seen.values(), "the image must show plane fronts and a plane back: %r" % seen
    both_ways(pkg, orc, ctx, scene)


def test_two_plane_nodes_with_different_chains(pkg, orc, ctx, tmp_path):
    """Matte planes (inline shading, no frame) with different chains side by side: one wavefront reads the tables of several plane nodes."""
    scene = load(pkg, tmp_path, NESTED % ("matte", "shiny") + OTHER_CHAIN, TWO_LIGHTS, CAM_ABOVE)
    both_ways(pkg, orc, ctx, scene)


def test_plane_with_a_zero_scale(pkg, orc, ctx, tmp_path):
    """A plane node and a parent whose scale is 0 on one axis: the inverse is not finite and the table holds what the arithmetic gives."""
    objects = """
      <object type="plane" name="flat" material="matte"><scale x="5" y="5" z="0"/><translate z="-1"/></object>
      <object name="g"><scale x="0" y="1" z="1"/>
        <object type="plane" name="gone" material="shiny"><scale value="3"/><translate z="0.5"/></object></object>
      <object type="plane" name="floor" material="matte"><scale value="12"/><translate z="-2"/></object>
    """
    scene = load(pkg, tmp_path, objects, TWO_LIGHTS, CAM_ABOVE)
    both_ways(pkg, orc, ctx, scene)


def test_planes_and_lights_follow_an_update(pkg, orc, tmp_path):
    """After rtu_update_scene has moved and rotated the planes' parent and changed a direct light, the image equals a fresh upload's."""
    scene = load(pkg, tmp_path, NESTED % ("matte", "mirror") + OTHER_CHAIN, TWO_LIGHTS, CAM_ABOVE)
    a, b = pkg.Context(0), pkg.Context(0)
    try:
        a.upload(scene)
        before = render(pkg, a, scene, False)
        scene.node_rotate(1, (0.3, 1.0, 0.2), 17.0)   # g1, the planes' outer parent (node 0 is the scene's root)
        scene.node_translate(1, (0.4, -0.3, 0.6))
        set_light_vec(scene, 2, (0.5, 0.1, -0.7))     # the direct light, not normalised
        a.update(scene)
        moved = both_ways(pkg, orc, a, scene, upload=False)
        assert not np.array_equal(bits(before), bits(moved)), "the update changed nothing"
        fresh = both_ways(pkg, orc, b, scene)
        assert np.array_equal(bits(moved), bits(fresh)), "an updated scene and a fresh upload differ"
    finally:
        a.close()
        b.close()


# ---- A: the direction of a direct light --------------------------------------------------------------------------------

BALLS = """
  <object type="sphere" name="ball" material="shiny"><translate x="-1" y="1" z="1"/></object>
  <object type="sphere" name="dull" material="matte"><scale value="1.5"/><translate x="3" y="2" z="1.5"/></object>
"""
FLOOR_AND_BALL = '<object type="plane" name="floor" material="matte"><scale value="15"/></object>' + BALLS
CAM_FLOOR = camera((2, -12, 6), (0.5, 0, 0.5))


def test_direct_light_directions(pkg, orc, ctx, tmp_path):
    """Three direct lights: axis-aligned (two exact zeros), one with a denormal component, one general."""
    lights = """
      <light type="direct" name="down"><intensity value="0.4"/><direction x="0" y="0" z="-1"/></light>
      <light type="direct" name="denormal"><intensity value="0.3"/><direction x="1e-40" y="0.6" z="-0.8"/></light>
      <light type="direct" name="general"><intensity value="0.3"/><direction x="-0.3" y="-0.2" z="-1"/></light>
    """
    scene = load(pkg, tmp_path, FLOOR_AND_BALL, lights, CAM_FLOOR)
    assert 0 < abs(lights_of(scene)[1].vec[0]) < 1.2e-38, "the loader kept no denormal component"
    both_ways(pkg, orc, ctx, scene)


@pytest.mark.parametrize("vec", [(3e-23, 0.0, -3e-23), (1e-30, 1e-30, -1e-30), (2e19, 1e19, -2e19), (0.0, 0.0, 0.0), (3.0, -4.0, -12.0)],
                         ids=["denormal-squares", "zero-length", "overflowing-length", "zero", "unnormalised"])
def test_direct_light_that_normalises_badly(pkg, orc, ctx, tmp_path, vec):
    """A direct light's vector as a caller may set it: squares that are denormal, underflow to zero (an infinite direction) or
    overflow (a zero direction), the zero vector (NaN) — the image holds what normalisation makes of each. Set by an update."""
    scene = load(pkg, tmp_path, FLOOR_AND_BALL, TWO_LIGHTS, CAM_FLOOR)
    ctx.upload(scene)
    before = render(pkg, ctx, scene, False)
    set_light_vec(scene, 2, vec)
    ctx.update(scene)
    after = both_ways(pkg, orc, ctx, scene, upload=False)
    assert not np.array_equal(bits(before), bits(after)), "the update of the light changed nothing"


# ---- C: the shadow ray's direction again -------------------------------------------------------------------------------

POINT_ONLY = """
  <light type="ambient" name="amb"><intensity value="0.1"/></light>
  <light type="point" name="pt"><intensity value="0.5"/><position x="0" y="0" z="5"/></light>
  <light type="point" name="pt2"><intensity value="0.3"/><position x="-6" y="-3" z="4"/></light>
"""


@pytest.mark.parametrize("where", ["1e-6 above a hit point", "at a hit point", "above a hit point's x and y", "1e6 away"])
def test_point_light_near_far_and_at_a_hit_point(pkg, orc, ctx, tmp_path, where):
    """A point light 1e-6 above a pixel's hit point on the floor, exactly at it (a zero vector: NaN direction), straight above it
    (two exactly zero components of light - point: subtraction is not antisymmetric there) and 1e6 away."""
    scene = load(pkg, tmp_path, FLOOR_AND_BALL, POINT_ONLY, CAM_FLOOR)
    hits = hit_points(pkg, orc, scene)
    y, x = 30, 20
    assert hits["node"][y, x] == 1 and hits["p"][y, x][2] == 0.0, "pixel (%d, %d) does not show the floor" % (x, y)
    p = hits["p"][y, x].astype(np.float64)
    pos = {"1e-6 above a hit point": (p[0], p[1], 1e-6), "at a hit point": (p[0], p[1], p[2]), "above a hit point's x and y": (p[0], p[1], 3.0),
           "1e6 away": (6e5, -5e5, 6e5)}[where]
    set_light_vec(scene, 1, pos, intensity={"1e-6 above a hit point": 1e-9, "1e6 away": 1e11}.get(where, 0.5))
    got = lights_of(scene)[1].vec
    if where != "1e6 away":
        assert np.float32(got[0]) == hits["p"][y, x][0] and np.float32(got[1]) == hits["p"][y, x][1]
    fast = both_ways(pkg, orc, ctx, scene)
    if where == "at a hit point":
        assert np.isnan(fast[y, x, :3]).all(), "the pixel whose hit point is the light's position is not NaN"


def test_point_light_behind_half_of_the_image(pkg, orc, ctx, tmp_path):
    """Two matte planes meeting in a valley, a point light below the left one: behind the surface for that half of the image (no
    shadow ray is fired there, the literal expression stays), in front of the right one; a matte sphere whose far side the
    lights do not see."""
    objects = """
      <object type="plane" name="left" material="matte"><scale value="8"/><rotate angle="35" y="1"/><translate x="-5"/></object>
      <object type="plane" name="right" material="matte"><scale value="8"/><rotate angle="-35" y="1"/><translate x="5"/></object>
      <object type="sphere" name="dull" material="matte"><scale value="1.5"/><translate x="0" y="-2" z="5"/></object>
    """
    lights = """
      <light type="point" name="low"><intensity value="0.8"/><position x="-9" y="0" z="-1"/></light>
      <light type="point" name="low2"><intensity value="0.5"/><position x="9" y="-3" z="7"/></light>
      <light type="direct" name="dir"><intensity value="0.3"/><direction x="1" y="0.2" z="-0.3"/></light>
    """
    scene = load(pkg, tmp_path, objects, lights, camera((0, -16, 12), (0, 0, 3)))
    fast = both_ways(pkg, orc, ctx, scene)
    hits = hit_points(pkg, orc, scene)
    assert {1, 2, 3} <= set(np.unique(hits["node"]).tolist())
    assert len(np.unique(bits(fast[..., :3]))) > 100  # a shaded image, not a constant


# ---- D: no view vector where no highlight is evaluated -----------------------------------------------------------------

MATTE_AND_SHINY_FLOOR = """
  <object type="plane" name="floor" material="matte"><scale value="15"/></object>
  <object type="plane" name="tile" material="shiny"><scale value="2"/><translate x="2.5" y="1" z="0.01"/></object>
"""


def test_light_along_the_view_direction(pkg, orc, ctx, tmp_path):
    """A matte floor seen from above with a direct light that shines from below, exactly against the view direction of a pixel near
    the image centre: there V + L is zero to rounding (the half vector is noise or NaN), around it cos^2(V, L) crosses 0.98 — where
    a test on the unnormalised view vector would hand over to the guard on the half vector —, and a specular tile in the same image
    evaluates its highlight. A second light from above."""
    lights = """
      <light type="direct" name="along"><intensity value="0.6"/><direction x="0" y="0" z="1"/></light>
      <light type="direct" name="above"><intensity value="0.5"/><direction x="0.2" y="0.1" z="-1"/></light>
      <light type="point" name="pt"><intensity value="0.4"/><position x="-3" y="2" z="6"/></light>
    """
    scene = load(pkg, tmp_path, MATTE_AND_SHINY_FLOOR, lights, camera((0.3, -0.2, 9), (0, 0, 0), up=(0, 1, 0), fov=40))
    fr = pkg.frame_setup(scene.desc.camera, W, H)
    rays = pkg.camera_rays(fr).reshape(H, W)
    y, x = H // 2, W // 2
    d = rays["dir"][y, x].astype(np.float64)
    set_light_vec(scene, 0, -d)  # lightDirection = normalize(-vec) = the ray's direction = -V at that pixel
    cos = -(rays["dir"].astype(np.float64) @ (d / np.linalg.norm(d)))   # cos(V, L) per pixel, to rounding
    assert (cos * cos > 0.98).sum() > 20 and (cos * cos < 0.98).sum() > 1000, "the image does not straddle the threshold"
    both_ways(pkg, orc, ctx, scene)


def test_camera_on_the_plane(pkg, orc, ctx, tmp_path):
    """The camera 1e-16 above a matte floor, looking along it and slightly down."""
    scene = load(pkg, tmp_path, MATTE_AND_SHINY_FLOOR + BALLS, TWO_LIGHTS, camera((0, -6, 1e-16), (0, 0, -0.4), fov=60))
    both_ways(pkg, orc, ctx, scene)


def test_eye_at_the_hit_point_of_a_ray_batch(pkg, orc, ctx, tmp_path):
    """rtu_shade_rays takes the eye apart from the rays: an eye 1e-16 from the hit points (v . v below the test's range), exactly at
    one (v = 0: NaN) and 1e16 away (above the range) — the view vector is normalised after all there."""
    scene = load(pkg, tmp_path, MATTE_AND_SHINY_FLOOR, TWO_LIGHTS, CAM_FLOOR)
    fr = pkg.frame_setup(scene.desc.camera, W, H)
    rays = pkg.camera_rays(fr)
    hits = orc.trace_rays(scene, rays, threads=4)
    floor = np.flatnonzero(hits["node"] == 1)  # (node 0 is the scene's root)
    assert floor.size > 1000 and (hits["node"] == 2).sum() > 50, "the rays must hit the matte floor and the specular tile"
    k = int(floor[floor.size // 2])
    p = hits["p"][k].astype(np.float64)
    ctx.upload(scene)
    for eye in [(p[0], p[1], 1e-16), (p[0], p[1], p[2]), (1e16, -1e16, 1e16), (p[0] + 1e-14, p[1], 2e-15)]:
        fast, _ = ctx.shade_rays(rays, eye)
        counting, _ = ctx.shade_rays(rays, eye, reference_walk=True)
        try:
            assert pkg.hip.rtu_debug_flags(ctx._h, LITERAL) == 0
            literal, _ = ctx.shade_rays(rays, eye)
        finally:
            pkg.hip.rtu_debug_flags(ctx._h, 0)
        assert np.array_equal(bits(fast), bits(counting)), "eye %r: fast and counting variants differ" % (eye,)
        assert np.array_equal(bits(fast), bits(literal)), "eye %r: the fast variant differs with debug flag 4096" % (eye,)
        cpu, _ = orc.shade_rays(scene, rays, eye, threads=4)
        check_against(fast.reshape(H, W, 4), cpu.reshape(H, W, 4), orc)
