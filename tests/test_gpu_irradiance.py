"""The irradiance map on the device (rtu_irradiance_build / rtu_render_frame_irradiance, include/rtu_render.h "Irradiance map") against
the chain of entries it is made of: rtu_irradiance_classify pass by pass (pure host code, itself checked against a numpy restatement
in tests/test_irradiance_host.py), rtu_gather_rays on M copies of each listed point's ray, rtu_trace_rays and the oracle's trace for
z and N; and the frame against camera sample rays, lookup at centres, ambient batch, sum in sample order.
The same against the oracle (rtu_oracle_rays_keyed's GATHER and AMBIENT, tests/test_oracle_rays_keyed.py): the chain run with the
oracle's gather gives the byte plane bit for bit — at thresholds chosen on the oracle alone, with a margin asserted there —, E and the
averages under the colour bar, and the frame is the oracle's ambient batches summed in sample order.
Shapes: 96x72 with (-4, -1) (a 49x37 grid, three levels), 24x10 with (-3, -1) (the ragged 13x6 grid) and 24x10 with min == max;
M = 4. Scene and camera: the recipe-P golden p13_p2_96x72."""
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_shade_rays_sampled import eye_of, same_bytes
from test_irradiance_host import field, run_pass
from test_oracle_rays_keyed import IRR_CASES, IRR_COLOUR_BAR, IRR_FIRST, IRR_M, IRR_MARGIN, IRR_TAG, oracle_irradiance_chain

pytestmark = pytest.mark.gpu

F = np.float32
M = 4
CASES = [(96, 72, -4, -1), (24, 10, -3, -1), (24, 10, -1, -1)]
# colour and depth thresholds that can refuse as well: E is of the order of 1, the room is 50 - 70 units deep
THR = dict(threshold_color=1.0, threshold_z=5.0, threshold_n=0.7)


@pytest.fixture(scope="module")
def ctx(pkg, golden):
    c = pkg.Context(0)
    c.upload(golden("p13_p2_96x72").scene(pkg))
    yield c
    c.close()


@pytest.fixture(scope="module")
def built(pkg, golden, ctx):
    """Per case, computed once and left unchanged: the frame, the descriptor, the device build and the rays of the grid points."""
    cache = {}

    def get(case, **thr):
        key = (case, tuple(sorted(thr.items())))
        if key not in cache:
            W, H, mn, mx = case
            scene = golden("p13_p2_96x72").scene(pkg)
            frame = pkg.frame_setup(scene.desc.camera, W, H)
            desc = pkg.irradiance_desc(min_subdiv=mn, max_subdiv=mx, samples=M, first_sample=3, **thr)
            rec, comp, per = ctx.irradiance_build(frame, desc)
            rays = pkg.irradiance_rays(frame, desc)
            for a in (rec, comp, per, rays):
                a.setflags(write=False)
            cache[key] = SimpleNamespace(scene=scene, frame=frame, desc=desc, rec=rec, comp=comp, per=per, rays=rays, W=W, H=H, mx=mx)
        return cache[key]
    return get


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_%d_%d" % c)
def test_the_device_build_is_the_host_chain(pkg, orc, ctx, built, case):
    b = built(case, **THR)
    gh, gw = b.comp.shape
    _, _, passes = pkg.irradiance_grid(b.desc, b.W, b.H)
    rec, comp = np.full((gh, gw, 8), F(-77.0), F), np.full((gh, gw), 9, np.uint8)
    eye = eye_of(b.frame)
    hits = ctx.trace_rays(b.rays)
    cpu = orc.trace_rays(b.scene, b.rays, threads=4)
    for p in range(passes):
        visit, compute = pkg.irradiance_classify(b.desc, b.W, b.H, p, rec, comp)
        want = visit[compute]
        assert (len(visit), len(want)) == tuple(b.per[p]), "pass %d: points visited and computed" % p
        if len(want):
            rays = np.repeat(b.rays[want], M)
            keys = np.array([pkg.sample_key(int(i), 3 + m) for i in want for m in range(M)], np.uint32)
            c = ctx.gather_rays(rays, keys, eye, max_bounce=b.desc.max_bounce)[0].reshape(len(want), M, 4)
            E = c[:, 0, :3].copy()
            for m in range(1, M):
                E = E + c[:, m, :3]  # float32, in the order of m
            E = E / F(M)
            flat = rec.reshape(-1, 8)
            flat[want, 0:3] = E
            flat[want, 3] = hits["t"][want]
            flat[want, 4:7] = hits["N"][want]
            flat[want, 7] = 0
            comp.reshape(-1)[want] = 1
            hit = (hits["flags"][want] & pkg.RTU_RAY_HIT) != 0
            flat[want[~hit], 4:7] = 0  # a miss stores N = 0 (and z = tmax, which is its t)
        print("%dx%d pass %d: %d visited, %d computed" % (b.W, b.H, p, len(visit), len(want)))
    assert same_bytes(comp, b.comp)
    assert same_bytes(rec, b.rec)
    # z and N of computed points: the bits of rtu_trace_rays, and so the oracle's
    done = b.comp.reshape(-1) == 1
    dev = b.rec.reshape(-1, 8)
    assert same_bytes(dev[done, 3], cpu["t"][done])
    hit = (cpu["flags"] & pkg.RTU_RAY_HIT) != 0
    assert same_bytes(dev[done & hit, 4:7], cpu["N"][done & hit]) and not dev[done & ~hit, 4:7].any()
    assert same_bytes(hits["t"], cpu["t"])
    if case[2] == case[3]:
        assert done.all()  # min == max computes every point
    elif case[:2] == (96, 72):
        assert done.any() and not done.all()  # (the 13x6 grid over this room estimates nothing at these thresholds; at the defaults it does, below)
    # the device form into the caller's memory: the same bytes
    import torch
    d_rec = torch.full((gh * gw * 8,), 5.0, dtype=torch.float32, device="cuda:0")
    d_comp = torch.full((gh * gw,), 7, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    per = ctx.irradiance_build_device(b.frame, b.desc, d_rec.data_ptr(), d_comp.data_ptr())
    assert np.array_equal(per, b.per)
    assert same_bytes(d_rec.cpu().numpy().reshape(gh, gw, 8), b.rec) and same_bytes(d_comp.cpu().numpy().reshape(gh, gw), b.comp)


@pytest.mark.parametrize("case", CASES[:2], ids=lambda c: "%dx%d_%d_%d" % c)
def test_default_thresholds_follow_the_oracles_normals(pkg, orc, ctx, built, case):
    """Colour and depth never refuse at the class's own thresholds (1e30), so which points are computed is a function of the first
    hits' normals alone: the numpy restatement of tests/test_irradiance_host.py run on the oracle's trace gives the byte plane."""
    b = built(case)
    d = pkg.irradiance_desc()
    assert list(b.desc.threshold_color) == list(d.threshold_color) and b.desc.threshold_z == d.threshold_z and b.desc.threshold_n == d.threshold_n
    gh, gw = b.comp.shape
    cpu = orc.trace_rays(b.scene, b.rays, threads=4)
    truth = field(gw, gh, gw, gh)  # (any finite E will do)
    truth[..., 3] = cpu["t"].reshape(gh, gw)
    truth[..., 4:7] = np.where(((cpu["flags"] & pkg.RTU_RAY_HIT) != 0)[:, None], cpu["N"], 0).reshape(gh, gw, 3)
    rec, comp = np.zeros((gh, gw, 8), F), np.full((gh, gw), 9, np.uint8)
    thr = [F(1e30)] * 4 + [F(0.7)]
    for p in range(len(b.per)):
        run_pass(rec, comp, truth, case[3] - case[2], p, thr)
    print("%dx%d: %d of %d points computed at the default thresholds" % (b.W, b.H, int(b.comp.sum()), b.comp.size))
    assert same_bytes(comp, b.comp)
    assert set(np.unique(b.comp)) == {0, 1}  # it holds both values


def test_the_frame_is_its_chain(pkg, ctx, built):
    case = CASES[0]
    b = built(case, **THR)
    S = 3
    frame = pkg.frame_setup(b.scene.desc.camera, b.W, b.H, samples=S)
    img = ctx.render_irradiance(frame, b.rec, b.mx)
    eye = eye_of(frame)
    centres = np.array([(x + 0.5, y + 0.5) for y in range(b.H) for x in range(b.W)], F)
    amb = pkg.irradiance_sample(b.rec, b.W, b.H, b.mx, centres)[:, :3]
    acc = np.zeros((b.W * b.H, 3), F)
    zsum, nhit = np.zeros(b.W * b.H, F), np.zeros(b.W * b.H, np.uint32)
    for k in range(S):
        rays, keys = pkg.camera_sample_rays(frame, k)
        out = ctx.shade_rays_ambient(rays, keys, amb, eye)[0]
        acc = acc + out[:, :3]
        hit = out[:, 3] != F(1e30)
        zsum = np.where(hit, zsum + out[:, 3], zsum)
        nhit += hit
    mean = acc / F(S)
    assert same_bytes(img[..., :3].reshape(-1, 3), mean)
    z = np.where(nhit > 0, zsum / np.maximum(nhit, 1).astype(F), F(1e30)).astype(F)
    assert same_bytes(img[..., 3].reshape(-1), z)
    # its z is the recipe-S frame's z
    plain = ctx.render(frame)[0]
    assert same_bytes(img[..., 3], plain[..., 3])
    # ... and the map's light is really in it
    assert (img[..., :3] > plain[..., :3]).any(axis=2).mean() > 0.5
    # the device form
    import torch
    d_rec = torch.from_numpy(np.ascontiguousarray(b.rec).copy()).to("cuda:0")
    d_img = torch.full((b.W * b.H * 4,), 3.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.render_irradiance_device(frame, d_rec.data_ptr(), b.mx, d_img.data_ptr())
    assert same_bytes(d_img.cpu().numpy().reshape(b.H, b.W, 4), img)
    # the lookup on the device is the host lookup
    d_xy = torch.from_numpy(centres.copy()).to("cuda:0")
    d_out = torch.zeros((len(centres) * 8,), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.irradiance_sample_device(d_rec.data_ptr(), b.W, b.H, b.mx, d_xy.data_ptr(), len(centres), d_out.data_ptr())
    torch.cuda.synchronize()
    assert same_bytes(d_out.cpu().numpy().reshape(-1, 8), pkg.irradiance_sample(b.rec, b.W, b.H, b.mx, centres))


# ---- against the oracle ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_built(pkg, orc, golden):
    """Per case of IRR_CASES, once: the oracle's chain (tests/test_oracle_rays_keyed.py)."""
    cache = {}

    def get(case):
        if case not in cache:
            assert (IRR_TAG, IRR_M, IRR_FIRST) == ("p13_p2_96x72", M, 3)
            b = oracle_irradiance_chain(pkg, orc, golden(IRR_TAG).scene(pkg), case, IRR_CASES[case])
            for a in (b.rec, b.comp, b.per):
                a.setflags(write=False)
            cache[case] = b
        return cache[case]
    return get


@pytest.mark.parametrize("case", list(IRR_CASES), ids=lambda c: "%dx%d_%d_%d" % c)
def test_the_device_build_is_the_oracles_chain(pkg, orc, ctx, oracle_built, case):
    """Measured on the MI355X (NOTEBOOK section 20): E and the averages differ from the oracle's by at most 3.7e-9 at the computed points of the 96x72 map (values up to 6.9) and by nothing at its averages and in the 24x10 map."""
    o = oracle_built(case)
    print("%dx%d: the closest tested colour difference is %.3g of its threshold away from it" % (o.W, o.H, o.margin))
    assert o.margin > IRR_MARGIN
    rec, comp, per = ctx.irradiance_build(o.frame, o.desc)
    assert set(np.unique(o.comp)) == {0, 1}  # both values occur
    assert np.array_equal(per, o.per), "points visited and computed per pass: %s vs the oracle chain's %s" % (per.tolist(), o.per.tolist())
    assert same_bytes(comp, o.comp), "the byte plane differs from the oracle chain's at %d points" % int((comp != o.comp).sum())
    assert same_bytes(rec[..., 3:], o.rec[..., 3:])  # z, N and the zero: bit for bit, computed or averaged
    for name, mask in (("E at computed points", o.comp == 1), ("the averages at estimated points", o.comp == 0)):
        d = np.abs(rec[mask][:, :3].astype(np.float64) - o.rec[mask][:, :3].astype(np.float64))
        print("%dx%d %s: %d points, largest |difference| %.3g, largest value %.3g" % (o.W, o.H, name, int(mask.sum()), d.max(), o.rec[mask][:, :3].max()))
        assert d.max() < IRR_COLOUR_BAR, "%s differ from the oracle's by %.3g" % (name, d.max())


def test_the_frame_against_the_oracle(pkg, orc, ctx, golden, oracle_built):
    """rtu_render_frame_irradiance on the oracle-built map against the oracle's ambient batches of the camera sample rays, summed in
    sample order in binary32: z bit for bit, colours under the bar of check() (tests/test_gpu_shade_rays_sampled.py)."""
    from test_gpu_shade_rays_sampled import check
    case = list(IRR_CASES)[0]
    o = oracle_built(case)
    S = 3
    W, H = o.W, o.H
    scene = golden(IRR_TAG).scene(pkg)
    frame = pkg.frame_setup(scene.desc.camera, W, H, samples=S)
    img = ctx.render_irradiance(frame, o.rec, o.mx)
    eye = eye_of(frame)
    centres = np.array([(x + 0.5, y + 0.5) for y in range(H) for x in range(W)], F)
    amb = pkg.irradiance_sample(o.rec, W, H, o.mx, centres)[:, :3]
    acc = np.zeros((W * H, 3), F)
    zsum, nhit = np.zeros(W * H, F), np.zeros(W * H, np.uint32)
    for k in range(S):
        rays, keys = pkg.camera_sample_rays(frame, k)
        out = orc.shade_rays_ambient(scene, rays, keys, amb, eye, threads=8)[0]
        acc = acc + out[:, :3]
        hit = out[:, 3] != F(1e30)
        zsum = np.where(hit, zsum + out[:, 3], zsum)
        nhit += hit
    want = np.empty((H, W, 4), F)
    want[..., :3] = (acc / F(S)).reshape(H, W, 3)
    want[..., 3] = np.where(nhit > 0, zsum / np.maximum(nhit, 1).astype(F), F(1e30)).astype(F).reshape(H, W)
    assert same_bytes(img[..., 3], want[..., 3]), "z differs from the oracle's"
    d = np.abs(img[..., :3].astype(np.float64) - want[..., :3].astype(np.float64))
    print("%dx%d frame with the map's light: largest |difference| %.3g, largest value %.3g" % (W, H, d.max(), want[..., :3].max()))
    check(img, want, orc, S, "the frame with the map's light")


def test_errors(pkg, golden):
    import ctypes
    scene = golden("p13_p2_96x72").scene(pkg)
    frame = pkg.frame_setup(scene.desc.camera, 24, 10, samples=2)
    desc = pkg.irradiance_desc(min_subdiv=-3, max_subdiv=-1, samples=M)
    ctx = pkg.Context(0)
    try:
        with pytest.raises(pkg.RtuError) as e:
            ctx.irradiance_build(frame, desc)
        assert e.value.code == pkg.RTU_ERR_NO_SCENE
        ctx.upload(scene)
        rec, comp, per = ctx.irradiance_build(frame, desc)
        for bad, code in ((pkg.irradiance_desc(min_subdiv=-3, max_subdiv=-2, samples=M), pkg.RTU_ERR_ARG),  # 10 is no multiple of 4
                          (pkg.irradiance_desc(min_subdiv=0, max_subdiv=1, samples=M), pkg.RTU_ERR_UNSUPPORTED),
                          (pkg.irradiance_desc(min_subdiv=-3, max_subdiv=-1, samples=0), pkg.RTU_ERR_ARG)):
            n = ctypes.c_uint32()
            assert pkg.hip.rtu_irradiance_build(ctx._h, ctypes.byref(frame), ctypes.byref(bad), rec.ctypes.data, comp.ctypes.data, ctypes.byref(n), None) == code
        sharded = pkg.frame_setup(scene.desc.camera, 24, 10, shard_rank=0, shard_count=2, samples=2)
        with pytest.raises(pkg.RtuError) as e:
            ctx.irradiance_build(sharded, desc)
        assert e.value.code == pkg.RTU_ERR_UNSUPPORTED
        with pytest.raises(pkg.RtuError) as e:
            ctx.render_irradiance(sharded, rec, -1)
        assert e.value.code == pkg.RTU_ERR_UNSUPPORTED
        for f in (pkg.frame_setup(scene.desc.camera, 24, 10), pkg.frame_setup(scene.desc.camera, 24, 10, samples=2, gather_bounces=4),
                  pkg.frame_setup(scene.desc.camera, 24, 12, samples=2)):
            with pytest.raises(pkg.RtuError) as e:  # recipe W; recipe P; a map of another size
                if f.height == 12:
                    m = pkg.RtuIrradianceMap()
                    m.width, m.height, m.max_subdiv, m.records = 24, 10, -1, rec.ctypes.data
                    out = np.zeros((12, 24, 4), F)
                    ctx._check(pkg.hip.rtu_render_frame_irradiance(ctx._h, ctypes.byref(f), ctypes.byref(m), out.ctypes.data))
                else:
                    ctx.render_irradiance(f, rec, -1)
            assert e.value.code == pkg.RTU_ERR_ARG
        with pytest.raises(pkg.RtuError) as e:
            ctx.render_irradiance(frame, rec, 1)
        assert e.value.code == pkg.RTU_ERR_UNSUPPORTED
        ctx.frame_status()
        assert same_bytes(ctx.irradiance_build(frame, desc)[0], rec)  # the context still works, and a build repeats itself
    finally:
        ctx.close()
