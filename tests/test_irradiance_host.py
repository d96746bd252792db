"""The irradiance map's pure host forms (rtu_irradiance_grid / _classify / _sample, include/rtu_render.h "Irradiance map") against a
numpy restatement of the rules, on synthetic record fields: a smooth colour ramp, a depth step and a normal crease.

Shapes: 2x2 with max = min = -1 (four border points, no refinement pass); 8x8 with (-3, 0) (a 9x9 grid that holds exactly one coarse
cell); 24x10 with (-3, -1) (a ragged 13x6 grid: the last cells are cut off); 67x35 with (-2, 0) (odd sizes, a 68x36 grid). The error
cases: 67x35 and 24x10 are no multiples of the spacing at max = -1 / -2.
(The issue lists 67x35 with (-2, 0) "as an error case"; at max_subdiv = 0 the spacing is one pixel and every size is a multiple, so
that shape is checked in full as a valid map, and 67x35 is the error case at max_subdiv = -1 and -2.)

Both branches of every refinement pass are exercised: the restatement itself estimates at least a tenth of the pass's points and
computes at least a tenth. Two passes cannot satisfy that whatever the field holds, and the test asserts exactly that about them:
level 1 of the 9x9 grid visits ONE cell centre, and its four edge midpoints all lie on the image border, where a point is always
computed."""
import ctypes

import numpy as np
import pytest

F = np.float32


def field(gw, gh, xs, yc):
    """records float32 [gh, gw, 8]: E a ramp, z a ramp with a step of 10 at x >= xs, N = +z below the crease y >= yc and +y above"""
    y, x = np.mgrid[0:gh, 0:gw]
    rec = np.zeros((gh, gw, 8), F)
    rec[..., 0] = F(0.1) + F(0.02) * x.astype(F) + F(0.01) * y.astype(F)
    rec[..., 1] = F(0.3) + F(0.005) * x.astype(F)
    rec[..., 2] = F(0.7) - F(0.01) * y.astype(F)
    rec[..., 3] = F(5.0) + F(0.1) * x.astype(F) + np.where(x >= xs, F(10.0), F(0.0)).astype(F)
    rec[..., 4:7] = np.where((y >= yc)[..., None], np.array([0, 1, 0], F), np.array([0, 0, 1], F))
    return rec


# ---- the numpy restatement -------------------------------------------------------------------------------------------------------
def grid_of(width, height, mn, mx):
    s = 1 << -mx
    assert width % s == 0 and height % s == 0
    return width // s + 1, height // s + 1, mx - mn


def pass_points(gw, gh, levels, p):
    """(phase, half, [(x, y)] in visiting order) of pass p"""
    if p == 0:
        skip = 1 << levels
        return 0, skip // 2, [(x, y) for y in range(0, gh, skip) for x in range(0, gw, skip)]
    level = (p + 1) // 2
    skip = 1 << (levels - level + 1)
    half = skip // 2
    if p % 2 == 1:
        return 1, half, [(x, y) for y in range(half, gh, skip) for x in range(half, gw, skip)]
    pts = []
    for y in range(0, gh, half):
        x0 = half if (y // half) % 2 == 0 else 0
        pts += [(x, y) for x in range(x0, gw, skip)]
    return 2, half, pts


def neighbours(gw, gh, phase, half, x, y):
    if phase == 0 or not (x + half < gw and y + half < gh):
        return None
    if phase == 1:
        return [(x - half, y - half), (x + half, y - half), (x - half, y + half), (x + half, y + half)]
    if x == 0 or y == 0:
        return None
    return [(x, y - half), (x - half, y), (x + half, y), (x, y + half)]


def estimate(rec, nb, thr):
    d = [rec[y, x] for x, y in nb]
    avg = (((d[0] + d[1]) + d[2]) + d[3]) * F(0.25)  # float32 arrays: one rounding per operation
    avg[7] = 0
    ok = True
    for r in d:
        dif = np.abs(avg[:4] - r[:4])
        dot = (avg[4] * r[4] + avg[5] * r[5]) + avg[6] * r[6]
        ok = ok and bool(dif[0] < thr[0] and dif[1] < thr[1] and dif[2] < thr[2] and dif[3] < thr[3] and dot > thr[4])
    return avg, ok


def run_pass(rec, comp, truth, levels, p, thr):
    """One pass of the restatement in place; a computed point takes the field's value. -> (visit indices, compute flags, estimable)"""
    gh, gw = comp.shape
    phase, half, pts = pass_points(gw, gh, levels, p)
    visit, flags, estimable = [], [], 0
    new = {}
    for x, y in pts:
        nb = neighbours(gw, gh, phase, half, x, y)
        est = False
        if nb is not None:
            estimable += 1
            avg, est = estimate(rec, nb, thr)
            if est:
                new[(x, y)] = avg
        visit.append(y * gw + x)
        flags.append(not est)
    for x, y in pts:  # (a pass reads earlier passes only: writing afterwards changes nothing, and shows it)
        if (x, y) in new:
            rec[y, x] = new[(x, y)]
            comp[y, x] = 0
        else:
            rec[y, x] = truth[y, x]
            comp[y, x] = 1
    return np.array(visit, np.uint32), np.array(flags, bool), estimable


def sample(rec, s, px, py):
    gh, gw = rec.shape[:2]
    iskip = F(1.0) / F(s)
    xx, yy = F(px) * iskip, F(py) * iskip
    ix, iy = int(xx), int(yy)
    fx, fy = xx - F(ix), yy - F(iy)
    ix2, iy2 = ix + 1, iy + 1
    if ix >= gw:
        ix = ix2 = gw - 1
    elif ix2 >= gw:
        ix2 = gw - 1
    if iy >= gh:
        iy = iy2 = gh - 1
    elif iy2 >= gh:
        iy2 = gh - 1
    one = F(1.0)
    lerp = lambda a, b, f: a * (one - f) + b * f
    return lerp(lerp(rec[iy, ix], rec[iy, ix2], fx), lerp(rec[iy2, ix], rec[iy2, ix2], fx), fy)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# (width, height, min, max, step at x >=, crease at y >=)
CASES = [(2, 2, -1, -1, 1, 1), (8, 8, -3, 0, 7, 7), (24, 10, -3, -1, 9, 5), (67, 35, -2, 0, 40, 20)]
THR = dict(threshold_color=(0.5, 0.5, 0.5), threshold_z=1.0, threshold_n=0.7)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_%d_%d" % c[:4])
def test_classify_against_the_restatement(pkg, case):
    W, H, mn, mx, xs, yc = case
    desc = pkg.irradiance_desc(min_subdiv=mn, max_subdiv=mx, **THR)
    gw, gh, levels = grid_of(W, H, mn, mx)
    assert pkg.irradiance_grid(desc, W, H) == (gw, gh, 1 + 2 * levels)
    if (W, H) == (24, 10):
        assert (gw, gh) == (13, 6)
    if (W, H) == (8, 8):
        assert (gw, gh) == (9, 9) and len(pass_points(gw, gh, levels, 0)[2]) == 4  # exactly one coarse cell
    truth = field(gw, gh, xs, yc)
    thr = [F(0.5), F(0.5), F(0.5), F(1.0), F(0.7)]
    poison = F(-77.0)
    rec_lib, comp_lib = np.full((gh, gw, 8), poison, F), np.full((gh, gw), 9, np.uint8)
    rec_np, comp_np = rec_lib.copy(), comp_lib.copy()
    written = np.zeros(gw * gh, int)
    for p in range(1 + 2 * levels):
        visit, flags, estimable = run_pass(rec_np, comp_np, truth, levels, p, thr)
        v_lib, f_lib = pkg.irradiance_classify(desc, W, H, p, rec_lib, comp_lib)
        assert np.array_equal(v_lib, visit), "pass %d: the order" % p
        assert np.all(np.diff(visit.astype(np.int64)) > 0)  # rising grid index: the list is in grid order
        assert np.array_equal(f_lib, flags), "pass %d: the decisions" % p
        # the library left the points it wants computed alone; the caller stores them
        want = v_lib[f_lib]
        assert np.all(bits(rec_lib.reshape(-1, 8)[want]) == bits(poison)) and np.all(comp_lib.reshape(-1)[want] == 9)
        rec_lib.reshape(-1, 8)[want] = truth.reshape(-1, 8)[want]
        comp_lib.reshape(-1)[want] = 1
        assert np.array_equal(bits(rec_lib), bits(rec_np)), "pass %d: the averages, bit for bit" % p
        assert np.array_equal(comp_lib, comp_np)
        written[visit] += 1
        n, est, com = len(visit), int((~flags).sum()), int(flags.sum())
        print("%dx%d (%d, %d) pass %d: %d points, %d estimable, %d estimated, %d computed" % (W, H, mn, mx, p, n, estimable, est, com))
        if p == 0:
            assert est == 0
        elif estimable < 2:
            assert (W, H) == (8, 8) and p in (1, 2)  # one centre; four border midpoints: no field can show both branches there
        else:
            assert 10 * est >= n and 10 * com >= n, "pass %d does not exercise both branches" % p
        # the always-computed border points of an edge pass
        if p and p % 2 == 0:
            vy, vx = np.divmod(visit, gw)
            half = pass_points(gw, gh, levels, p)[1]
            border = (vx == 0) | (vy == 0) | (vx + half >= gw) | (vy + half >= gh)
            assert border.any() and flags[border].all()
    assert np.all(written == 1), "every point of the grid is written exactly once"
    assert set(np.unique(comp_lib)) <= {0, 1} and not np.any(bits(rec_lib[..., :7]) == bits(poison))
    if levels == 0:
        assert np.all(comp_lib == 1)
    with pytest.raises(pkg.RtuError):
        pkg.irradiance_classify(desc, W, H, 1 + 2 * levels, rec_lib, comp_lib)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_%d_%d" % c[:4])
def test_lookup_against_the_restatement(pkg, case):
    W, H, mn, mx, xs, yc = case
    gw, gh, _ = grid_of(W, H, mn, mx)
    s = 1 << -mx
    rec = field(gw, gh, xs, yc)
    rng = np.random.default_rng(5)
    centres = [(x + 0.5, y + 0.5) for y in range(H) for x in range(W)][:: max(1, W * H // 200)]
    edge = [(W - 0.5, 0.5), (0.5, H - 0.5), (W - 0.5, H - 0.5), (float(W), float(H)), (W - 1e-3, H - 1e-3), (0.0, 0.0)]
    beyond = [(W + 0.25, 1.5), (1.5, H + 0.75), (W + 3.5, H + 9.25), (3.0 * W, 0.5), (0.5, 1000.0)]
    rnd = list(zip(rng.uniform(0, W, 50), rng.uniform(0, H, 50)))
    xy = np.array(centres + edge + beyond + rnd, F)
    out = pkg.irradiance_sample(rec, W, H, mx, xy)
    ref = np.stack([sample(rec, s, px, py) for px, py in xy])
    assert np.array_equal(bits(out), bits(ref))
    # at a grid point the lookup returns the point; beyond the last row and column, the last point
    assert np.array_equal(bits(pkg.irradiance_sample(rec, W, H, mx, [(float(W), float(H))])[0]), bits(rec[gh - 1, gw - 1]))
    far = pkg.irradiance_sample(rec, W, H, mx, [(W + 5.0 * s, H + 7.0 * s)])[0]
    assert np.allclose(far, rec[gh - 1, gw - 1], rtol=1e-6, atol=1e-6)
    # a negative or NaN coordinate is taken as 0
    neg = pkg.irradiance_sample(rec, W, H, mx, [(-3.0, float("nan"))])[0]
    assert np.array_equal(bits(neg), bits(rec[0, 0]))
    assert pkg.irradiance_sample(rec, W, H, mx, np.zeros((0, 2), F)).shape == (0, 8)


def test_descriptor_rules(pkg):
    d = pkg.irradiance_desc()
    assert (d.min_subdiv, d.max_subdiv, d.samples, d.first_sample, d.max_bounce) == (-5, 0, 64, 0, 5)
    assert list(d.threshold_color) == [F(1e30)] * 3 and d.threshold_z == F(1e30) and d.threshold_n == F(0.7)
    assert ctypes.sizeof(pkg.RtuIrradianceDesc) == 64 and ctypes.sizeof(pkg.RtuIrradianceMap) == 32
    assert pkg.irradiance_grid(d, 1920, 1080) == (1921, 1081, 11)

    def code(desc, W, H):
        return pkg.hip.rtu_irradiance_grid(ctypes.byref(desc), W, H, None, None, None)
    # not a multiple of the spacing
    assert code(pkg.irradiance_desc(min_subdiv=-2, max_subdiv=0), 67, 35) == pkg.RTU_OK
    assert code(pkg.irradiance_desc(min_subdiv=-2, max_subdiv=-1), 67, 35) == pkg.RTU_ERR_ARG
    assert code(pkg.irradiance_desc(min_subdiv=-2, max_subdiv=-2), 67, 35) == pkg.RTU_ERR_ARG
    assert code(pkg.irradiance_desc(min_subdiv=-3, max_subdiv=-1), 24, 10) == pkg.RTU_OK
    assert code(pkg.irradiance_desc(min_subdiv=-3, max_subdiv=-2), 24, 10) == pkg.RTU_ERR_ARG  # 10 is no multiple of 4
    assert code(pkg.irradiance_desc(min_subdiv=-3, max_subdiv=-2), 24, 12) == pkg.RTU_OK
    # several points per pixel
    assert code(pkg.irradiance_desc(min_subdiv=0, max_subdiv=1), 8, 8) == pkg.RTU_ERR_UNSUPPORTED
    assert code(pkg.irradiance_desc(min_subdiv=-1, max_subdiv=-2), 8, 8) == pkg.RTU_ERR_ARG
    for bad in (dict(samples=0), dict(samples=4097), dict(first_sample=-1), dict(max_bounce=6), dict(max_bounce=-1), dict(min_subdiv=-16),
                dict(threshold_z=float("nan")), dict(threshold_color=(1.0, float("nan"), 1.0))):
        assert code(pkg.irradiance_desc(**bad), 8, 8) == pkg.RTU_ERR_ARG, bad
    r = pkg.irradiance_desc()
    r.reserved[3] = 1
    assert code(r, 8, 8) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_irradiance_grid(None, 8, 8, None, None, None) == pkg.RTU_ERR_ARG
    assert code(d, 0, 8) == pkg.RTU_ERR_ARG
    with pytest.raises(pkg.RtuError):
        pkg.irradiance_sample(np.zeros((6, 13, 8), F), 24, 10, -2, [(1.0, 1.0)])


def test_the_rays_go_through_pixel_corners(pkg):
    cam = pkg.RtuCamera()
    cam.pos[:] = [0, -10, 2]
    cam.dir[:] = [0, 1, 0]
    cam.up[:] = [0, 0, 1]
    cam.fov = 40.0
    cam.focaldist = 1.0
    cam.img_width, cam.img_height = 24, 10
    frame = pkg.frame_setup(cam, 24, 10)
    desc = pkg.irradiance_desc(min_subdiv=-3, max_subdiv=-1)
    rays = pkg.irradiance_rays(frame, desc)
    assert rays.shape == (13 * 6,)
    o, u, v, c = (np.array(list(a), F) for a in (frame.origin, frame.u, frame.v, frame.cam_pos))
    for i in (0, 5, 13, 77):
        y, x = divmod(i, 13)
        cp = (o + u * F(F(x) * F(2.0))) + v * F(F(y) * F(2.0))
        d = cp - c
        d = d / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], dtype=F)
        assert np.array_equal(bits(rays["dir"][i]), bits(d)) and np.array_equal(bits(rays["org"][i]), bits(c))
    # the centre ray of pixel (0, 0) lies inside the cone of the four corner rays around it
    centre = pkg.camera_rays(frame, 0, 1)["dir"][0].astype(np.float64)
    one = pkg.irradiance_rays(frame, pkg.irradiance_desc(min_subdiv=0, max_subdiv=0))["dir"].astype(np.float64).reshape(11, 25, 3)
    corners = one[0:2, 0:2].reshape(4, 3)
    assert (corners @ centre).min() > (corners @ corners.T).min()
