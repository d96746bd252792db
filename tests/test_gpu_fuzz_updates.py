"""rtu_update_scene and rtu_update_meshes on the random scenes of tests/test_gpu_fuzz.py: up to five mesh nodes of two meshes, at node
depth up to four, instanced under nested non-uniform scales, lights dropped into the object box.

The edit script and the chain of deformations come from tests/test_fuzz_host.py, which asserts without a GPU that they give the
builders work (usable and unusable (light, mesh node) pairs, images that change). After every step the occluder lists the GPU built
equal the host builder's, the mesh structures equal the host restatement, and the updated context renders, bit for bit, what a context
that uploaded the edited scene afresh renders — which meets the oracle's image (8-bit +-1, linear RGB to INSIDE_GLASS_REL_TOL of
tests/test_gpu_fuzz.py: the edits and deformations put the camera's rays inside glass too), counters equal."""
import numpy as np
import pytest

from test_fuzz_host import TWO_MESH_SEEDS, W_SEEDS, edit_script, edit_step, mesh_script, w_scene
from test_gpu_fuzz import INSIDE_GLASS_REL_TOL, assets, rel_error  # noqa: F401  (assets: the fixture)
from test_gpu_mesh_update import check_update_against_upload_and_oracle
from test_gpu_parity import check_against
from test_gpu_scene_update import assert_lists_equal, same_bits
from test_mesh_update_host import assert_same_structures, clone, deformed_scene

pytestmark = pytest.mark.gpu

W, H = 96, 64


@pytest.fixture(scope="module")
def pair(pkg):
    a, b = pkg.Context(0), pkg.Context(0)
    yield a, b
    a.close()
    b.close()


def images(pkg, ctx, scene):
    """(the counting variant's image, its counters, the fast variant's images with stage 2 cooperative and one lane per ray)."""
    cnt, st = ctx.render(pkg.frame_setup(scene.desc.camera, W, H, collect_stats=True), stats=True)
    fast = []
    for thr in (10 ** 9, 1):
        fr = pkg.frame_setup(scene.desc.camera, W, H)
        fr.coop_threshold = thr
        fast.append(ctx.render(fr)[0])
    return cnt, st, fast


@pytest.mark.parametrize("seed", W_SEEDS)
def test_random_scene_updates(pkg, orc, pair, assets, seed):  # noqa: F811
    a, b = pair
    scene = w_scene(pkg, assets, seed)
    a.upload(scene)
    usable = 0
    for step, now in enumerate(edit_script(pkg, scene, seed)):
        what = "seed %d step %d" % (seed, step)
        a.update(now)
        b.upload(now)
        usable += assert_lists_equal(pkg, a, now, what)
        ca, sa, fa = images(pkg, a, now)
        cb, sb, fb = images(pkg, b, now)
        assert same_bits(ca, cb) and sa == sb, what + ": the updated context's counting variant differs from a fresh upload's"
        for k, thr in enumerate(("cooperative", "one lane per ray")):
            assert same_bits(fa[k], fb[k]), "%s: the updated context renders another image than a fresh upload (stage 2 %s)" % (what, thr)
            assert same_bits(fa[k], ca), "%s: fast (%s) and counting variants differ" % (what, thr)
        cpu, cst = orc.render(now, W, H, threads=8)
        print("%s: linear RGB differs by %.3g of max(|value|, 1e-3), largest value %.3g" % ((what,) + rel_error(ca, cpu, 1e-3)))
        check_against(ca, cpu, orc, rel_tol=INSIDE_GLASS_REL_TOL)
        assert sa == cst, what + ": counters differ from the oracle's"
    print("seed %d: %d lists compared" % (seed, usable))


@pytest.mark.parametrize("seed", TWO_MESH_SEEDS)
def test_random_scene_mesh_updates(pkg, orc, pair, assets, seed):  # noqa: F811
    a, b = pair
    scene = w_scene(pkg, assets, seed)
    assert scene.desc.n_meshes == 2
    a.upload(scene)

    def settle(now, what):
        for m in (0, 1):  # the mesh the call did not list as well: it must be what it was
            assert_same_structures(a.mesh_arrays(m), pkg.host_mesh(scene, m, now), "%s, mesh %d" % (what, m))
        assert_lists_equal(pkg, a, now, what)
        return check_update_against_upload_and_oracle(pkg, orc, a, b, now, what, shards=False, rel_tol=INSIDE_GLASS_REL_TOL)

    for now, ids, name in mesh_script(pkg, scene):
        a.update_meshes(now, ids)
        settle(now, "seed %d, %s" % (seed, name))
    # a scene edit, then a deformation, before one render
    edited = clone(pkg, now)
    edit_step(pkg, edited, np.random.RandomState(9000 + seed))
    a.update(edited)
    last = deformed_scene(pkg, edited, 0, ("twist", 120))
    a.update_meshes(last, [0])
    settle(last, "seed %d, an edit and a twist of mesh 0" % seed)
