"""rtu_trace_rays, rtu_occluded_rays and rtu_shade_rays on the random scenes of tests/test_gpu_fuzz.py, with rays no camera fires: the
families R1-R4 of tests/test_fuzz_host.py (from inside the object box, from surfaces, from outside and from under the floor, tmax
around the hit), which asserts on the oracle alone that each contains what it is meant to.

Every batch goes through check_batch of tests/test_gpu_rays_oracle.py: every field of the closest hit bit for bit, the occlusion byte,
t of the radiance bit for bit, NaN colours at the same rays, counters equal, the reference walk byte-identical to the fast walk in all
three entries. The colours: 8-bit +-1 and linear RGB to 1e-3 of max(|value|, 1e-3) — not test_random_scene's 1e-4, which rays that start
inside glass cannot meet (INSIDE_GLASS_REL_TOL in tests/test_gpu_fuzz.py says why). A sorted batch (sort=True) answers with the same bytes."""
import numpy as np
import pytest

from test_fuzz_host import W_SEEDS, eye_of, ray_families, w_scene
from test_gpu_fuzz import INSIDE_GLASS_REL_TOL, assets  # noqa: F401  (assets: the fixture)
from test_gpu_ray_query import same_hits
from test_gpu_rays_oracle import check_batch

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("seed", W_SEEDS)
def test_random_scene_rays(pkg, orc, ctx, assets, seed):  # noqa: F811
    scene = w_scene(pkg, assets, seed)
    fam = ray_families(pkg, orc, scene, seed)
    eye = eye_of(scene)
    ctx.upload(scene)
    for name, rays in fam:
        hit = check_batch(pkg, orc, ctx, scene, rays, eye, "seed %d %s" % (seed, name), rel_tol=INSIDE_GLASS_REL_TOL)
        assert hit.any()
    r1 = fam[0][1]
    assert same_hits(ctx.trace_rays(r1, sort=True), ctx.trace_rays(r1)), "sorted closest hits differ"
    assert np.array_equal(ctx.occluded(r1, sort=True), ctx.occluded(r1)), "sorted occlusion bytes differ"
    a, b = ctx.shade_rays(r1, eye, sort=True)[0], ctx.shade_rays(r1, eye)[0]
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "sorted radiance differs"
