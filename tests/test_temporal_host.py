"""The temporal accumulator's host form (rtu_temporal_accumulate, include/rtu_render.h "Temporal accumulation") — the executable
statement of the rules, which the device form must reproduce bit for bit (tests/test_gpu_temporal.py) — against an independent numpy
restatement of the same rules over chains of five frames, and its effect on the oracle's own path-traced samples along a camera
orbit. No GPU.

The restatement works on whole float32 arrays, one tap at a time in the order of the rules, so every pixel sees the same binary32
operations in the same order as tp_pixel of raytracer-utah_amd/csrc/rtu_temporal.h."""
import ctypes
import math

import numpy as np
import pytest

from test_denoise_host import SIZES, bits, dot3, make_inputs, oracle_guides
from test_mesh_update_host import clone

F = np.float32
RTU_RAY_HIT = 1
FRAMES = 5


def cross3(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)


def v3(x):
    return np.array(list(x), F)


def same_camera(a, b):
    return (a.width, a.height) == (b.width, b.height) and all(
        np.array_equal(bits(v3(getattr(a, k))), bits(v3(getattr(b, k)))) for k in ("cam_pos", "origin", "u", "v"))


def np_temporal(prev_cam, cur_cam, rgbz, hits, albedo, hist_prev, desc):
    """The rules of include/rtu_render.h restated: (rgbz_out [H, W, 4], history [3, H, W, 4], counts of the branches taken)."""
    H, W = rgbz.shape[:2]
    c = rgbz[..., :3]
    valid = (hits["flags"].reshape(H, W) & RTU_RAY_HIT) != 0
    a = albedo.reshape(H, W, 4)[..., :3]
    d = np.where(a > F(0.01), a, F(1.0))
    Np, Pp = hits["N"].reshape(H, W, 3), hits["p"].reshape(H, W, 3)
    t, node = hits["t"].reshape(H, W), hits["node"].reshape(H, W)
    normal_min, maxh = F(desc.normal_min), F(desc.max_history)
    acc, nacc, wsum = np.zeros((H, W, 3), F), np.zeros((H, W), F), np.zeros((H, W), F)
    ntaps, looked = np.zeros((H, W), int), np.zeros((H, W), bool)
    yg, xg = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        e_cur = c / d
        plane_max = F(desc.sigma_plane) * t

        def tap(qx, qy, w, mask):
            nonlocal acc, nacc, wsum, ntaps
            inside = mask & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            Eq, Pq, Nq = hist_prev[0][cy, cx], hist_prev[1][cy, cx], hist_prev[2][cy, cx]
            ok = inside & (Eq[..., 3] > 0) & (np.ascontiguousarray(Nq[..., 3]).view(np.int32) == node)
            ok &= dot3(Np, Nq[..., :3]) >= normal_min
            ok &= np.abs(dot3(Np, Pq[..., :3] - Pp)) <= plane_max
            acc = np.where(ok[..., None], acc + Eq[..., :3] * w[..., None], acc)
            nacc = np.where(ok, nacc + Eq[..., 3] * w, nacc)
            wsum = np.where(ok, wsum + w, wsum)
            ntaps += ok
        if hist_prev is None:
            pass
        elif same_camera(prev_cam, cur_cam):
            looked = valid.copy()
            tap(xg, yg, np.ones((H, W), F), looked)
        else:
            pos, origin, u, v = (v3(getattr(prev_cam, k)) for k in ("cam_pos", "origin", "u", "v"))
            nrm = cross3(u, v)
            num = dot3(origin - pos, nrm)
            D = Pp - pos
            s = num / dot3(D, nrm)
            m = np.isfinite(s) & (s > 0)
            Q = (pos + D * s[..., None]) - origin
            fx = dot3(Q, u) / dot3(u, u) - F(0.5)
            fy = dot3(Q, v) / dot3(v, v) - F(0.5)
            assert fx.dtype == F and num.dtype == F
            looked = valid & m & (fx >= F(-1.0)) & (fx < F(W)) & (fy >= F(-1.0)) & (fy < F(H))
            flx, fly = np.floor(np.where(looked, fx, F(0))), np.floor(np.where(looked, fy, F(0)))
            x0, y0 = flx.astype(int), fly.astype(int)
            wx, wy = fx - flx, fy - fly
            ux, uy = F(1.0) - wx, F(1.0) - wy
            tap(x0, y0, ux * uy, looked)
            tap(x0 + 1, y0, wx * uy, looked)
            tap(x0, y0 + 1, ux * wy, looked)
            tap(x0 + 1, y0 + 1, wx * wy, looked)
        has = valid & (wsum > F(0.01))
        e_prev = np.where(has[..., None], acc / wsum[..., None], F(0.0))
        n_prev = np.where(has, nacc / wsum, F(0.0))
        fin = np.isfinite(c).all(axis=-1)
        n_b = np.where(maxh < n_prev + F(1.0), maxh, n_prev + F(1.0))
        e_b = e_prev + (e_cur - e_prev) * (F(1.0) / n_b)[..., None]
        fresh = n_prev == 0
        e = np.where(~fin[..., None], e_prev, np.where(fresh[..., None], e_cur, e_b))
        n = np.where(~fin, n_prev, np.where(fresh, F(1.0), n_b))
        passthrough = ~valid | (~fin & fresh)
        out = rgbz.copy()
        out[..., :3] = np.where(passthrough[..., None], c, e * d)
    hist = np.zeros((3, H, W, 4), F)
    keep = valid & ~(~fin & fresh)
    hist[0][..., :3] = np.where(keep[..., None], e, F(0.0))
    hist[0][..., 3] = np.where(keep, n, F(0.0))
    hist[1][..., :3] = np.where(valid[..., None], Pp, F(0.0))
    hist[1][..., 3] = np.where(valid, t, F(0.0))
    hist[2][..., :3] = np.where(valid[..., None], Np, F(0.0))
    hist[2][..., 3] = np.where(valid, node, -1).astype(np.int32).view(F)
    assert out.dtype == F and e.dtype == F and n.dtype == F
    lk = looked & valid
    counts = {"taps0": int((lk & (ntaps == 0)).sum()), "taps1to3": int((lk & (ntaps >= 1) & (ntaps <= 3)).sum()),
              "taps4": int((lk & (ntaps == 4)).sum()), "small_wsum": int((lk & (ntaps > 0) & ~(wsum > F(0.01))).sum()),
              "clamped": int((valid & fin & ~fresh & (maxh < n_prev + F(1.0))).sum()), "carried": int((valid & ~fin & ~fresh).sum()),
              "dropped": int((valid & ~fin & fresh).sum()), "no_lookup": int((valid & ~looked).sum()),
              "off_left": 0, "off_right": 0, "off_top": 0, "off_bottom": 0}
    if hist_prev is not None and not same_camera(prev_cam, cur_cam):
        counts.update(off_left=int((lk & (x0 < 0)).sum()), off_right=int((lk & (x0 + 1 >= W)).sum()),
                      off_top=int((lk & (y0 < 0)).sum()), off_bottom=int((lk & (y0 + 1 >= H)).sum()))
    return out, hist, counts


def make_camera(pkg, W, H, pos=(0.0, 0.0, 0.0), shift=(0.0, 0.0), yaw=0.0):
    """The camera the synthetic hit points of make_inputs belong to — its image plane is their plane z = -5, one pixel per 0.1 —
    moved to `pos` + shift and turned by `yaw` radians about its own y axis."""
    f = pkg.RtuFrameDesc()
    f.width, f.height, f.shard_count, f.samples = W, H, 1, 1
    p = np.array(pos, np.float64) + np.array([shift[0], shift[1], 0.0])
    c, s = math.cos(yaw), math.sin(yaw)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    f.cam_pos[:] = [float(x) for x in p]
    f.origin[:] = [float(x) for x in p + R @ np.array([-0.05 * W - 0.05, -0.05 * H - 0.05, -5.0])]
    f.u[:] = [float(x) for x in R @ np.array([0.1, 0.0, 0.0])]
    f.v[:] = [float(x) for x in R @ np.array([0.0, 0.1, 0.0])]
    return f


def chain_cameras(pkg, W, H):
    """Two chains of five cameras. X: an equal camera (the static path), then previous cameras to the right / below and to the left /
    above, so that taps fall off each border. Y: a previous camera behind the surfaces (s <= 0), then a small rotation."""
    base = make_camera(pkg, W, H)
    A = make_camera(pkg, W, H, shift=(0.23, 0.11))
    B = make_camera(pkg, W, H, shift=(-0.37, -0.29), yaw=0.004)
    C = make_camera(pkg, W, H, pos=(0.0, 0.0, -20.0))
    R = make_camera(pkg, W, H, shift=(0.05, -0.02), yaw=-0.03)
    return {"X": [base, make_camera(pkg, W, H), A, B, A], "Y": [B, C, base, R, base]}


def chain_inputs(pkg, W, H, seed):
    """Five frames of make_inputs (tests/test_denoise_host.py: two planes meeting at an edge, a depth step, invalid pixels in blobs and
    singly, a NaN normal) on the same surfaces with other noise and other invalid pixels each; added here: a second node id across a
    coplanar seam, and samples with a NaN and with an infinite channel."""
    frames = []
    for k in range(FRAMES):
        rgbz, hits, albedo = make_inputs(pkg, W, H, seed + 17 * k)
        y = np.arange(W * H) // W
        valid = (hits["flags"] & RTU_RAY_HIT) != 0
        hits["node"] = np.where(valid, np.where(y < H // 3, 2, 1), -1)
        vi = np.flatnonzero(valid)
        if W * H > 1:
            flat = rgbz.reshape(-1, 4)
            for j, i in enumerate(vi[3::max(1, len(vi) // 6)]):
                flat[i, j % 3] = F(np.nan) if j % 2 == 0 else F(np.inf)
        frames.append((rgbz, hits, albedo))
    return frames


def run_chain(pkg, cams, frames, desc, form):
    """form(prev_cam, cur_cam, rgbz, hits, albedo, hist_prev, desc) -> (out, hist, ...) over the chain: [(out, hist)] per frame."""
    res, hist = [], None
    for k in range(FRAMES):
        r = form(cams[k - 1] if k else None, cams[k], *frames[k], hist, desc)
        hist = r[1]
        res.append(r)
    return res


def host_form(pkg):
    return lambda prev, cur, rgbz, hits, albedo, hist, desc: pkg.temporal_accumulate(prev, cur, rgbz, hits, albedo, hist, desc)


CHAINS = [("X", {"max_history": 3}), ("Y", {}), ("X", {"sigma_plane": 0.4, "normal_min": -1.0, "max_history": 2})]


# ---- 1. the host form against the numpy restatement, bit for bit --------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_host_form_equals_the_numpy_restatement(pkg, size):
    W, H = size
    total = {}
    for ci, (name, over) in enumerate(CHAINS):
        cams = chain_cameras(pkg, W, H)[name]
        frames = chain_inputs(pkg, W, H, 4321 + ci)
        desc = pkg.temporal_desc(W, H, **over)
        got = run_chain(pkg, cams, frames, desc, host_form(pkg))
        want = run_chain(pkg, cams, frames, desc, np_temporal)
        for k in range(FRAMES):
            for what, g, w in (("image", got[k][0], want[k][0]), ("history", got[k][1], want[k][1])):
                diff = bits(g) != bits(w)
                assert not diff.any(), "chain %s %s frame %d %s: %d words differ, first at %s" % (name, over, k, what, diff.sum(), np.argwhere(diff)[0])
            rgbz, hits = frames[k][0], frames[k][1]
            invalid = ((hits["flags"] & RTU_RAY_HIT) == 0).reshape(H, W)
            assert np.array_equal(bits(got[k][0])[invalid], bits(rgbz)[invalid]), "an invalid pixel was changed"
            assert np.array_equal(bits(got[k][0][..., 3]), bits(rgbz[..., 3])), "z was changed"
            h = got[k][1]
            assert not h[0][invalid].any() and not h[1][invalid].any() and not h[2][invalid][:, :3].any()
            assert (np.ascontiguousarray(h[2][..., 3]).view(np.int32)[invalid] == -1).all()
            for key, v in want[k][2].items():
                total[key] = total.get(key, 0) + v
            if name == "Y" and k == 2:  # the previous camera lies behind every surface
                assert want[k][2]["no_lookup"] == int((~invalid).sum()) and (h[0][..., 3][~invalid & np.isfinite(rgbz[..., :3]).all(-1)] == 1).all()
            if k == 0:
                assert set(np.unique(h[0][..., 3])) <= {0.0, 1.0}
    print(size, total)
    if size == (67, 35):  # every branch of the rules occurs
        for key in ("taps0", "taps1to3", "taps4", "small_wsum", "clamped", "carried", "dropped", "no_lookup", "off_left", "off_right", "off_top",
                    "off_bottom"):
            assert total[key] > 0, "no pixel took the branch %r: %s" % (key, total)


def test_static_camera_is_exact(pkg):
    """Equal cameras: no resampling — a pixel's history is its own, so the chain is the running mean of its samples."""
    W, H = 67, 35
    cams = [make_camera(pkg, W, H) for _ in range(FRAMES)]
    frames = chain_inputs(pkg, W, H, 99)
    first = frames[0]
    frames = [(f[0], first[1], first[2]) for f in frames]  # the same guides every frame
    res = run_chain(pkg, cams, frames, pkg.temporal_desc(W, H), host_form(pkg))
    valid = ((first[1]["flags"] & RTU_RAY_HIT) != 0).reshape(H, W)
    ok = valid & np.all([np.isfinite(f[0][..., :3]).all(-1) for f in frames], axis=0) & ~np.isnan(first[1]["N"]).any(-1).reshape(H, W)
    ok &= (first[1]["N"] != 0).any(-1).reshape(H, W)
    assert ok.sum() > 1000
    assert (res[-1][1][0][..., 3][ok] == FRAMES).all()


def test_in_place_defaults_and_refusals(pkg):
    W, H = 67, 35
    d = pkg.temporal_desc()
    assert (d.max_history, d.flags, ctypes.sizeof(d)) == (32, 0, 32) and d.sigma_plane == F(0.05) and d.normal_min == F(0.9)
    cams = chain_cameras(pkg, W, H)["X"]
    frames = chain_inputs(pkg, W, H, 5)
    res = run_chain(pkg, cams, frames, pkg.temporal_desc(W, H), host_form(pkg))
    rgbz, hits, albedo = frames[3]
    prev_hist = np.ascontiguousarray(res[2][1])
    d = pkg.temporal_desc(W, H)
    buf, hist = rgbz.copy(), np.empty((3, H, W, 4), F)

    def call(desc=d, prev=cams[2], cur=cams[3], a=None, hp=prev_hist.ctypes.data, ho=None, out=None):
        a = a or [buf.ctypes.data, hits.ctypes.data, albedo.ctypes.data]
        return pkg.hip.rtu_temporal_accumulate(ctypes.byref(desc) if desc is not None else None, ctypes.byref(prev) if prev is not None else None,
                                               ctypes.byref(cur) if cur is not None else None, a[0], a[1], a[2], hp,
                                               ho if ho is not None else hist.ctypes.data, out if out is not None else buf.ctypes.data)
    assert call() == pkg.RTU_OK                       # rgbz_out == rgbz
    assert np.array_equal(bits(buf), bits(res[3][0])) and np.array_equal(bits(hist), bits(res[3][1]))
    buf[:] = rgbz
    # aliased histories: the same buffer, and any overlap
    assert call(ho=prev_hist.ctypes.data) == pkg.RTU_ERR_ARG
    big = np.zeros(2 * prev_hist.size, F)
    big[:prev_hist.size] = prev_hist.reshape(-1)
    assert call(hp=big.ctypes.data, ho=big.ctypes.data + 16) == pkg.RTU_ERR_ARG
    assert call(hp=big.ctypes.data, ho=big.ctypes.data + 4 * prev_hist.size) == pkg.RTU_OK
    for bad in ({"max_history": 0}, {"max_history": 65536}, {"sigma_plane": 0.0}, {"sigma_plane": float("nan")}, {"normal_min": 1.5},
                {"normal_min": -1.01}, {"normal_min": float("nan")}, {"flags": 2}, {"width": 0}, {"height": -1}, {"width": 66}):
        bd = pkg.temporal_desc(W, H)
        for k, v in bad.items():
            setattr(bd, k, v)
        assert call(desc=bd) == pkg.RTU_ERR_ARG, bad
    for k in range(2):
        bd = pkg.temporal_desc(W, H)
        bd.reserved[k] = 1
        assert call(desc=bd) == pkg.RTU_ERR_ARG
    assert call(desc=pkg.temporal_desc(W, H, denoise=True)) == pkg.RTU_OK  # the session's flag is not the accumulator's business
    assert call(desc=None) == pkg.RTU_ERR_ARG and call(cur=None) == pkg.RTU_ERR_ARG and call(prev=None) == pkg.RTU_ERR_ARG
    assert call(prev=None, hp=None) == pkg.RTU_OK     # no history: no previous camera needed
    assert call(prev=make_camera(pkg, W + 1, H)) == pkg.RTU_ERR_ARG
    args = [buf.ctypes.data, hits.ctypes.data, albedo.ctypes.data]
    for k in range(3):
        assert call(a=[None if j == k else x for j, x in enumerate(args)]) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_temporal_accumulate(ctypes.byref(d), ctypes.byref(cams[2]), ctypes.byref(cams[3]), *args, None, None, buf.ctypes.data) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_temporal_accumulate(ctypes.byref(d), ctypes.byref(cams[2]), ctypes.byref(cams[3]), *args, None, hist.ctypes.data, None) == pkg.RTU_ERR_ARG


# ---- 2. quality, on the oracle alone ---------------------------------------------------------------------------------------------
ORBIT_FRAMES = 8
ORBIT_STEP_DEG = 0.25


def orbit_scene(pkg, scene, k, distance, step_deg=ORBIT_STEP_DEG):
    """`scene` with its camera turned k * step_deg degrees about its up axis around its target, the point pos + dir * distance."""
    s = clone(pkg, scene)
    cam = s.desc.camera
    pos, d, up = (np.array(list(x), np.float64) for x in (cam.pos, cam.dir, cam.up))
    d /= np.linalg.norm(d)
    up /= np.linalg.norm(up)
    target = pos + d * distance
    a = math.radians(k * step_deg)
    r = pos - target
    r = r * math.cos(a) + np.cross(up, r) * math.sin(a) + up * np.dot(up, r) * (1 - math.cos(a))
    new_pos = target + r
    cam.pos[:] = [float(x) for x in new_pos]
    cam.dir[:] = [float(x) for x in (target - new_pos) / np.linalg.norm(target - new_pos)]
    return s


# RMSE over all pixels, linear rgb, of the last of eight frames (an orbit of 8 x 0.25 degrees: 99.9 % of the pixels end with n >= 2,
# at 0.5 degrees the last cameras see past the room's open side) against 256 spp of the last camera, p11_p2_120x68, the defaults:
# measured 0.02402 for the raw last sample, ratio 0.287 accumulated and 0.212 with the filter on top. The bounds are those ratios
# times 1.25, rounded up to two digits.
ACC_BOUND = 0.36
DN_BOUND = 0.27


def test_quality_on_the_oracle(pkg, orc, golden):
    g = golden("p11_p2_120x68")
    scene = g.scene(pkg)
    W, H = g.width, g.height
    desc = pkg.temporal_desc(W, H)
    hist, prev, out = None, None, None
    centre = oracle_guides(pkg, orc, scene, W, H)[0][(H // 2) * W + W // 2]
    assert centre["flags"] & RTU_RAY_HIT
    for k in range(ORBIT_FRAMES):
        s = orbit_scene(pkg, scene, k, float(centre["t"]))  # the target: what the centre of the golden image shows
        frame = pkg.frame_setup(s.desc.camera, W, H, samples=16, gather_bounces=4)
        sample = orc.sample_images(s, W, H, 16, k, 1, gi=True, threads=8)[0]
        hits, albedo = oracle_guides(pkg, orc, s, W, H)
        assert ((hits["flags"] & RTU_RAY_HIT) != 0).all(), "a closed room: every pixel hits"
        out, hist = pkg.temporal_accumulate(prev, frame, sample, hits, albedo, hist, desc)
        prev = frame
    n = hist[0][..., 3]
    share = float((n >= 2).mean())
    print("orbit of %d x %.2f deg: %.1f %% of the pixels have n >= 2, mean n %.2f" % (ORBIT_FRAMES, ORBIT_STEP_DEG, 100 * share, n.mean()))
    assert share >= 0.8, "the orbit's step is too large for this test: a condition on its input"
    ref = orc.render_paths(s, W, H, 256, threads=8)[0]

    def rmse(img):
        return float(np.sqrt(np.mean((img[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)) ** 2)))
    raw = rmse(sample)
    acc = rmse(out) / raw
    dn = rmse(pkg.denoise(out, hits, albedo)) / raw
    print("RMSE raw %.5f, accumulated ratio %.3f, accumulated and filtered ratio %.3f" % (raw, acc, dn))
    assert acc < ACC_BOUND, "accumulated: RMSE ratio %.3f" % acc
    assert dn < DN_BOUND, "accumulated and filtered: RMSE ratio %.3f" % dn
