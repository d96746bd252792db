"""The host side of rtu_update_scene, no GPU: the Scene mutators (rtu_scene_node_scale / _rotate / _translate, rtu_scene_set_light)
against the loader itself, and the shape check (rtu_scene_shape_diff) field by field."""
import ctypes

import pytest

from test_light_lists import RtuLight, RtuNode

XML = """<xml><scene>
  <object name="g">{g}
    <object type="obj" name="{o}" material="m">{t}</object></object>
  <object type="sphere" name="s" material="m"><scale value="0.5"/><translate x="3"/></object>
  <material type="blinn" name="m"><diffuse r="0.6" g="0.6" b="0.6"/></material>
  <light type="point" name="p"><intensity value="0.5"/><position x="4" y="-6" z="5"/></light>
  <light type="direct" name="d"><intensity value="0.3"/><direction {d}/></light>
</scene><camera><position x="0" y="-20" z="6"/><target x="0" y="0" z="1"/><up x="0" y="0" z="1"/><fov value="45"/>
  <width value="64"/><height value="48"/></camera></xml>"""
BASE_G = '<rotate angle="25" x="1" y="0.3" z="0.2"/><translate x="1" y="-2" z="3"/>'
BASE_T = '<scale x="1.5" y="0.7" z="2.0"/><rotate angle="40" z="1"/><translate x="-2" z="1"/>'
BASE_D = 'x="1" y="0.2" z="-0.05"'


@pytest.fixture
def load(pkg, tmp_path):
    from test_gpu_parity import _write_uv_mesh
    _write_uv_mesh(tmp_path / "m.obj", 6, 4, lambda u, v: (u, v, u * v))

    def get(g=BASE_G, t=BASE_T, d=BASE_D):
        xml = tmp_path / "s.xml"
        xml.write_text(XML.format(g=g, t=t, d=d, o=tmp_path / "m.obj"))
        return pkg.Scene.from_xml(str(xml))
    return get


def node_bytes(scene):
    n = ctypes.cast(scene.desc.nodes, ctypes.POINTER(RtuNode))
    return [bytes(n[i]) for i in range(scene.desc.n_nodes)]


def light_bytes(scene):
    lights = ctypes.cast(scene.desc.lights, ctypes.POINTER(RtuLight))
    return [bytes(lights[i]) for i in range(scene.desc.n_lights)]


@pytest.mark.parametrize("node", [1, 2])
def test_node_operations_equal_the_loader(load, node):
    ops = [("rotate", ((0.3, -1.0, 0.5), 33.0), '<rotate angle="33" x="0.3" y="-1" z="0.5"/>'),
           ("scale", ((1.25, 0.5, 2.0),), '<scale x="1.25" y="0.5" z="2"/>'),
           ("translate", ((0.75, -1.5, 2.25),), '<translate x="0.75" y="-1.5" z="2.25"/>'),
           ("rotate", ((0.0, 0.0, 2.0), -70.0), '<rotate angle="-70" z="2"/>')]
    scene = load()
    xml = ""
    for name, args, tag in ops:
        if name == "rotate":
            scene.node_rotate(node, *args)
        elif name == "scale":
            scene.node_scale(node, *args[0])
        else:
            scene.node_translate(node, args[0])
        xml += tag
        want = load(g=BASE_G + xml, t=BASE_T) if node == 1 else load(g=BASE_G, t=BASE_T + xml)
        assert node_bytes(scene) == node_bytes(want), "after %s" % name


def test_set_light_equals_the_loader(load):
    scene = load()
    want = load(d='x="-3" y="0.5" z="-2"')
    lights = ctypes.cast(scene.desc.lights, ctypes.POINTER(RtuLight))
    l = RtuLight.from_buffer_copy(bytes(lights[1]))
    l.vec[0], l.vec[1], l.vec[2] = -3.0, 0.5, -2.0  # not normalised: set_light does it as DirectLight::SetDirection
    scene.set_light(1, l)
    assert light_bytes(scene) == light_bytes(want)
    p = RtuLight.from_buffer_copy(bytes(lights[0]))
    p.vec[0] = 7.5
    p.size = 0.25
    scene.set_light(0, p)
    assert bytes(lights[0]) == bytes(p)  # a point light's position is taken as it is


def test_mutators_refuse_bad_indices(pkg, load):
    scene = load()
    with pytest.raises(pkg.RtuError):
        scene.node_rotate(99, (0, 0, 1), 10)
    with pytest.raises(pkg.RtuError):
        scene.node_translate(scene.desc.n_nodes, (0, 0, 1))
    with pytest.raises(pkg.RtuError):
        scene.set_light(scene.desc.n_lights, RtuLight())


class RtuTexture(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("rgb", ctypes.c_void_p), ("color1", ctypes.c_float * 3), ("color2", ctypes.c_float * 3)]


def clone(pkg, scene):
    return pkg.Scene(pkg.host.rtu_scene_clone(scene.desc_ptr))


def test_shape_check_names_every_field(pkg, golden):
    scene = golden("p7_200x150").scene(pkg)  # textured, with material maps
    assert pkg.scene_shape_diff(scene, scene) is None
    other = clone(pkg, scene)
    # placement, lights and materials are not shape
    other.node_rotate(2, (0, 1, 0), 30)
    other.node_translate(1, (1, 2, 3))
    lights = ctypes.cast(other.desc.lights, ctypes.POINTER(RtuLight))
    lights[1].vec[0] += 1.0
    lights[1].type = 2
    assert pkg.scene_shape_diff(scene, other) is None
    d = other.desc
    n = ctypes.cast(d.nodes, ctypes.POINTER(RtuNode))
    meshes = ctypes.cast(d.meshes, ctypes.POINTER(pkg.RtuMesh))
    tex = ctypes.cast(d.textures, ctypes.POINTER(RtuTexture))
    cases = [(n[2], f, "node 2: " + f) for f in ("parent", "obj_type", "mesh_id", "depth", "subtree_end")]
    cases += [(meshes[0], f, "mesh 0: " + f) for f in ("nv", "nf", "nvn", "nvt", "n_bvh_nodes")]
    cases += [(d, f, f) for f in ("n_nodes", "n_meshes", "n_textures", "n_materials")]
    for obj, field, want in cases:
        old = getattr(obj, field)
        setattr(obj, field, old - 1 if field.startswith("n_") else old + 1)
        got = pkg.scene_shape_diff(scene, other)
        setattr(obj, field, old)
        assert got is not None and want in got, (field, got)
    for name in ("type", "width", "height"):
        old = getattr(tex[1], name)
        setattr(tex[1], name, old + 1)
        got = pkg.scene_shape_diff(scene, other)
        setattr(tex[1], name, old)
        assert got is not None and "texture 1: " + name in got, got
    maps = d.material_maps
    d.material_maps = None
    got = pkg.scene_shape_diff(scene, other)
    d.material_maps = maps
    assert got is not None and "material_maps" in got
    assert pkg.scene_shape_diff(scene, other) is None


def test_scene_shape_error_text(pkg):
    assert pkg.hip.rtu_error_string(pkg.RTU_ERR_SCENE_SHAPE).decode() == "scene shape differs from the uploaded scene"
    assert "scene shape differs" in str(pkg.RtuError(pkg.RTU_ERR_SCENE_SHAPE, "node 1: parent differs"))


def test_update_needs_a_context(pkg, golden):
    scene = golden("teapot2_240x135").scene(pkg)
    assert pkg.hip.rtu_update_scene(None, scene.desc_ptr) == pkg.RTU_ERR_ARG
