"""rtu_update_meshes_device on the meshes of tests/golden/ref_trees: what the GPU builds must be the tree the COMPILED REFERENCE built
for the same vertices (test_ref_trees_host.py holds the host side to those fixtures) — and on soups of exactly 64, 128, 256 faces and
their neighbours, where a wave of the builder's folds is exactly full, has a one-lane tail, or a block boundary is crossed.

A fixture F is a scene the reference flattened. The context uploads a copy of it with OTHER vertices, then takes F's vertices from
device memory; afterwards it must hold what rtu_debug_host_mesh states for F — whose `ref` tree and element order are the bytes of
the reference's blob, renumbered breadth-first. All comparisons are exact. Where a mesh makes NaN triangle records or normals (nan, inf,
huge, collapse), WHICH NaN an operation returns is the processor's choice (see test_gpu_mesh_update_device.py test_nan_vertices): there a
NaN equals a NaN and every other word is exact."""
import numpy as np
import pytest

from test_gpu_mesh_update import render
from test_gpu_mesh_update_device import assert_shape_is, check_structures, device_update, on_device, raw_update
from test_gpu_parity import check_against
from test_gpu_scene_update import assert_lists_equal, same_bits
from test_mesh_update_host import RTU_MAX_BVH_STACK, assert_same_structures, clone, same_bits_nan
from test_ref_build_host import obj_scene, soup, vn_of
from test_ref_trees_host import FIXTURE_IDS, FIXTURES, H, W, fixture_scene, stale_copy

pytestmark = pytest.mark.gpu

NAN_RECORDS = ("nan", "inf", "huge", "collapse")  # meshes with NaN triangle records or normals
RENDERED = ("flat60", "grid", "signed_zero")
REFUSED = ("deep60",)  # the one fixture deeper than the walk's stack


@pytest.fixture(scope="module")
def ctx(pkg):
    """One context for every fixture, in turn: the builder's scratch always holds the previous mesh's contents."""
    c = pkg.Context(0)
    yield c
    c.close()


def assert_structures_nan_is_nan(got, want, what):
    """assert_same_structures where a NaN of the records or normals equals any NaN and every other word is exact; returns the number
    of NaN words."""
    nans = 0
    for key in ("fast_tri", "ref_tri", "vn"):
        assert same_bits_nan(got[key], want[key]), "%s: %s differs" % (what, key)
        nans += int(np.isnan(want[key]).sum())
    loose = dict(got)
    loose["vn"] = want["vn"]  # (compared above)
    assert_same_structures(loose, want, what, strict_nan=False)
    return nans


@pytest.mark.parametrize("name,kind", FIXTURES, ids=FIXTURE_IDS)
def test_fixture_through_the_device_path(pkg, orc, ctx, name, kind):
    F = fixture_scene(pkg, name, kind)
    what = "%s_%s" % (name, kind)
    base = stale_copy(pkg, F)
    ctx.upload(base)
    t = on_device(F.mesh_vertices(0))
    if name in REFUSED:
        assert F.mesh(0).bvh_depth == 57 > RTU_MAX_BVH_STACK
        held = ctx.mesh_arrays(0)
        before, bst = render(pkg, ctx, base, stats=True)
        assert raw_update(pkg, ctx, base, [(0, t.data_ptr())]) == pkg.RTU_ERR_UNSUPPORTED
        assert "depth" in pkg.hip.rtu_last_error(ctx._h).decode()
        assert_same_structures(ctx.mesh_arrays(0), held, what + " refused", strict_nan=True)
        assert_shape_is(ctx, base, 0, what + " refused")
        after, ast = render(pkg, ctx, base, stats=True)
        assert same_bits(before, after) and bst == ast, what + ": the refused call changed the image"
        return
    if name in RENDERED:
        before, _ = render(pkg, ctx, base)
    ctx.update_meshes_device(base, {0: (t.data_ptr(), None, kind == "c")})
    got, want = ctx.mesh_arrays(0), pkg.host_mesh(base, 0, F)
    if name in NAN_RECORDS:
        print("%s: %d NaN words among records and normals" % (what, assert_structures_nan_is_nan(got, want, what)))
    else:
        assert_same_structures(got, want, what, strict_nan=True)
    assert_shape_is(ctx, F, 0, what)
    assert_lists_equal(pkg, ctx, F, what)
    if kind == "c":
        vn = vn_of(F, 0)
        same = same_bits_nan(got["vn"], vn) if name in NAN_RECORDS else np.array_equal(got["vn"].view(np.uint32), vn.view(np.uint32))
        assert same, what + ": normals differ from the reference's ComputeNormals"
    if name in RENDERED:
        cnt, gstats = render(pkg, ctx, F, stats=True)
        fast, _ = render(pkg, ctx, F)
        assert same_bits(cnt, fast), what + ": fast and counting variants differ"
        assert not same_bits(fast, before), what + ": the update did not change the image"
        cpu, cstats = orc.render(F, W, H, threads=8)
        assert np.array_equal(cnt[..., 3].view(np.uint32), cpu[..., 3].view(np.uint32)), what + ": z differs from the oracle's"
        assert gstats == cstats, "%s: counters differ from the oracle's: %s vs %s" % (what, gstats, cstats)
        check_against(cnt, cpu, orc)


# ---- wave and block edges -------------------------------------------------------------------------------------------------------------

# 1024 first: every scratch buffer is then larger than any later use and holds an earlier mesh's contents
EDGE_SIZES = [1024, 63, 257, 64, 256, 65, 255, 128]


def test_wave_and_block_edges(pkg, tmp_path):
    assert sorted(EDGE_SIZES) == [63, 64, 65, 128, 255, 256, 257, 1024]
    ctx = pkg.Context(0)
    try:
        for n in EDGE_SIZES:
            v, f = soup(n, n)
            v2 = soup(n, n + 100)[0]
            for normals in (True, False):
                what = "soup of %d faces, %s" % (n, "vn lines" if normals else "normals recomputed")
                scene = obj_scene(pkg, tmp_path, "soup%d%s" % (n, "n" if normals else "c"), v, f, normals)
                now = clone(pkg, scene)
                now.set_mesh_vertices(0, v2)
                if not normals:
                    now.recompute_normals(0)
                ctx.upload(scene)
                device_update(ctx, scene, now, [0], recompute=not normals)
                check_structures(pkg, ctx, scene, now, [0], what)
        # the vertex box folds over nv: 64 faces and one loose vertex are three full waves and a tail of one lane
        v, f = soup(64, 64)
        loose = np.array([[9, -9, 9]], np.float32)
        scene = obj_scene(pkg, tmp_path, "soup64_loose", np.concatenate([v, loose]), f)
        assert scene.mesh(0).nv == 193
        now = clone(pkg, scene)
        now.set_mesh_vertices(0, np.concatenate([soup(64, 164)[0], -loose]))
        ctx.upload(scene)
        device_update(ctx, scene, now, [0])
        check_structures(pkg, ctx, scene, now, [0], "soup of 64 faces and a loose vertex")
        assert ctx.mesh_shape(0).bound_min[0] == -9 and ctx.mesh_shape(0).bound_max[1] == 9
    finally:
        ctx.close()
