"""Temporal accumulation for sensors (include/rtu_render.h, "Temporal accumulation for sensors"), the part that needs no GPU: the
projection rtu_sensor_project of the three models against a numpy binary32 restatement of the header's expressions — with its own
float64 fdlibm acos — bit for bit, its round trip through rtu_sensor_rays, the host accumulators rtu_temporal_accumulate_sensor and
_sensor_moments against a numpy restatement of the rules, a panorama's pure yaw followed across the seam on the oracle's guides, the
STATIC path against the camera forms, and every refusal.

The restatements work on whole float32 arrays, one operation at a time in the order of the rules, so every element sees the binary32
operations of sensor_project (rtu_sensor.h) and tp_pixel (rtu_temporal.h) in their order."""
import ctypes
import math

import numpy as np
import pytest

from test_denoise_host import bits, dot3
from test_sensor_host import MODELS, camera_basis, make
from test_temporal_host import FRAMES, chain_inputs, make_camera

F = np.float32
RTU_RAY_HIT = 1
SIZES = [(64, 32), (33, 17), (48, 48), (40, 30)]
TWO_PI, PI, HALF_PI = F(6.2831855), F(3.1415927), F(1.5707964)


def v3(x):
    return np.array(list(x), F)


# ---- the restatement of the projection ---------------------------------------------------------------------------------------------
def np_acos(xf):
    """portable_acos: fdlibm's e_acos in float64 IEEE operations, rounded to float32."""
    pio2_hi, pio2_lo, pi = 1.57079632679489655800e+00, 6.12323399573676603587e-17, 3.14159265358979311600e+00

    def poly(z):
        p = z * (1.66666666666666657415e-01 + z * (-3.25565818622400915405e-01 + z * (2.01212532134862925881e-01 +
            z * (-4.00555345006794114027e-02 + z * (7.91534994289814532176e-04 + z * 3.47933107596021167570e-05)))))
        q = 1.0 + z * (-2.40339491173441421878e+00 + z * (2.02094576023350569471e+00 + z * (-6.88283971605453293030e-01 + z * 7.70381505559019352791e-02)))
        return p / q
    x = np.asarray(xf, F).astype(np.float64)
    ax = np.abs(x)
    with np.errstate(all="ignore"):
        small = pio2_hi - (x - (pio2_lo - x * poly(x * x)))
        zn = (1.0 + x) * 0.5
        sn = np.sqrt(zn)
        neg = pi - 2.0 * (sn + (poly(zn) * sn - pio2_lo))
        zp = (1.0 - x) * 0.5
        sp = np.sqrt(zp)
        pos = 2.0 * (sp + poly(zp) * sp)
    r = np.where(ax >= 1.0, np.where(x > 0, 0.0, pi), np.where(ax < 0.5, small, np.where(x < 0, neg, pos)))
    return r.astype(F)


ACOS_ARGS = []  # every argument np_angle hands to np_acos, for the check against the oracle's portable_acos


def np_angle(s, k):
    """angle(s, k) of the header: (the angle, whether there is one)."""
    with np.errstate(all="ignore"):
        L = np.sqrt(s * s + k * k)
        ok = np.isfinite(L) & (L > 0)
        direct = np.abs(k) <= s
        arg = np.where(direct, k / L, s / L)
        ACOS_ARGS.append(arg[ok].reshape(-1))
        q = np_acos(arg)
        ang = np.where(direct, q, np.where(k > 0, HALF_PI - q, HALF_PI + q))
    assert L.dtype == F and ang.dtype == F
    return ang, ok


def np_project(d, P):
    """sensor_project restated: world points P float32 [..., 3] -> (fx, fy, ok) in sensor d."""
    W, H = F(d.width), F(d.height)
    with np.errstate(all="ignore"):
        Q = P - v3(d.pos)
        a, b, c = dot3(Q, v3(d.forward)), dot3(Q, v3(d.right)), dot3(Q, v3(d.up))
        if d.model == 0:
            h = np.sqrt(a * a + b * b)
            pol, ok1 = np_angle(h, c)
            th, ok2 = np_angle(np.abs(b), -a)
            lon = np.where(b <= 0, th, TWO_PI - th)
            fx = lon / TWO_PI * W - F(0.5)
            fy = pol / PI * H - F(0.5)
            ok = (h != 0) & ok1 & ok2
        elif d.model == 1:
            p = np.sqrt(b * b + c * c)
            ang, ok1 = np_angle(p, a)
            r = ang / F(F(d.fov_deg) * F(0.008726646))
            R = F(F(0.5) * F(min(d.width, d.height)))
            fx = ((r * (b / p)) * R + F(0.5) * W) - F(0.5)
            fy = ((-(r * (c / p))) * R + F(0.5) * H) - F(0.5)
            centre = p == 0
            fx = np.where(centre, F(0.5) * W - F(0.5), fx)
            fy = np.where(centre, F(0.5) * H - F(0.5), fy)
            ok = np.where(centre, a > 0, ok1 & (r <= 1))
        else:
            fx = (b / F(d.extent[0]) + F(0.5)) * W - F(0.5)
            fy = (F(0.5) - c / F(d.extent[1])) * H - F(0.5)
            ok = a > 0
    assert fx.dtype == F and fy.dtype == F and a.dtype == F
    return fx, fy, ok


def project64(d, P):
    """The same projection in float64 with arctan2, on the same float32 inputs: (fx, fy)."""
    Q = P.astype(np.float64) - np.array(list(d.pos), np.float64)
    fwd, right, up = (np.array(list(v), np.float64) for v in (d.forward, d.right, d.up))
    a, b, c = Q @ fwd, Q @ right, Q @ up
    W, H = d.width, d.height
    with np.errstate(all="ignore"):
        if d.model == 0:
            lon = np.arctan2(-b, -a) % (2 * math.pi)
            pol = np.arctan2(np.hypot(a, b), c)
            return lon / (2 * math.pi) * W - 0.5, pol / math.pi * H - 0.5
        if d.model == 1:
            p = np.hypot(b, c)
            r = np.arctan2(p, a) / math.radians(d.fov_deg / 2)
            R = 0.5 * min(W, H)
            return r * b / p * R + 0.5 * W - 0.5, -r * c / p * R + 0.5 * H - 0.5
        return (b / d.extent[0] + 0.5) * W - 0.5, (0.5 - c / d.extent[1]) * H - 0.5


def frame_of(d):
    return (v3(d.pos).astype(np.float64), v3(d.right).astype(np.float64), v3(d.up).astype(np.float64), v3(d.forward).astype(np.float64))


def special_points(d):
    """Points on the sensor's axes, behind it, at both poles, on the seam (b = +-0 with a < 0), on the fisheye's rim and at its centre."""
    pos, right, up, fwd = frame_of(d)
    pts = [pos, pos + fwd, pos - fwd, pos + right, pos - right, pos + up, pos - up, pos + 3 * up, pos - 7 * up,
           pos - 2 * fwd + 0.0 * right, pos - 2 * fwd + 1e-30 * right, pos - 2 * fwd - 1e-30 * right,
           pos + 2.5 * fwd, pos + 1e-3 * fwd, pos + fwd + 1e-8 * right]
    half = math.radians(d.fov_deg / 2)
    for phi in np.linspace(0, 2 * math.pi, 9):  # the rim of a fisheye, from both sides
        for da in (-1e-3, 0.0, 1e-7, 1e-3):
            pts.append(pos + 2 * (math.cos(half + da) * fwd + math.sin(half + da) * (math.cos(phi) * right + math.sin(phi) * up)))
    return np.array(pts, np.float64).astype(F)


def points_for(d, seed):
    rng = np.random.default_rng(seed)
    pos = v3(d.pos)
    rnd = (pos + rng.normal(0, 1, (4000, 3)) * rng.choice([0.01, 1.0, 50.0], (4000, 1))).astype(F)
    odd = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [1e38, 1e38, -1e38], [0, 0, 0]], F)
    return np.concatenate([rnd, special_points(d), odd])


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("model", MODELS)
def test_projection_equals_the_restatement(pkg, orc, model, size):
    W, H = size
    ACOS_ARGS.clear()
    for k, d in enumerate((make(pkg, model, W, H, fov_deg=140.0), make(pkg, model, W, H, fov_deg=360.0, extent=(0.7, 5.0), pos=(0.0, 0.0, 0.0)),
                           pkg.sensor_desc(model, W, H, (1.0, 2.0, 3.0), (1, 0, 0), (0, 1, 0), (0, 0, -1), fov_deg=90.0, extent=(2.0, 2.0)))):
        P = points_for(d, 100 * k + W)
        if k == 2:  # an axis frame: b, c and a are exact, so these ARE the pole, the seam with b = +0 and b = -0, and the fisheye's centre
            pos = v3(d.pos)
            P = np.concatenate([P, pos + np.array([[0, 2, 0], [0, -2, 0], [0.0, 0, 3], [-0.0, 0, 3], [0, 0.5, 3], [0, 0, -4], [0, 0, 4],
                                                   [1, 0, 0], [-1, 0, 0], [1, 0, -1], [0, 1, -1]], F)])
        fxfy, ok = pkg.sensor_project(d, P)
        fx, fy, want_ok = np_project(d, P)
        assert np.array_equal(ok, want_ok), "%s: ok differs at %s" % (model, np.flatnonzero(ok != want_ok)[:5])
        assert ok.sum() > 100
        for name, g, w in (("fx", fxfy[:, 0], fx), ("fy", fxfy[:, 1], fy)):
            diff = (bits(g) != bits(w)) & ok
            assert not diff.any(), "%s %s sensor %d: %d differ, first point %s: %r != %r" % (model, name, k, diff.sum(), P[diff][0], g[diff][0], w[diff][0])
        assert not fxfy[~ok].any(), "a point without an image answers (0, 0)"
        if k == 2:
            n0 = len(P) - 11
            sp = dict(zip(("pole+", "pole-", "seam+0", "seam-0", "seam_up", "centre", "behind"), range(n0, n0 + 7)))
            if model == "equirect":
                assert not ok[sp["pole+"]] and not ok[sp["pole-"]] and ok[sp["seam+0"]] and ok[sp["seam-0"]]
                # b <= 0 holds for both zeros: the seam is lon = 0, column -0.5, for either sign
                assert fxfy[sp["seam+0"], 0] == F(-0.5) and fxfy[sp["seam-0"], 0] == F(-0.5)
                assert fxfy[sp["centre"], 0] == F(0.5 * W - 0.5) and fxfy[sp["centre"], 1] == F(0.5 * H - 0.5)
            elif model == "fisheye":
                assert ok[sp["centre"]] and not ok[sp["behind"]] and tuple(fxfy[sp["centre"]]) == (F(0.5 * W - 0.5), F(0.5 * H - 0.5))
            else:
                assert ok[sp["centre"]] and not ok[sp["behind"]] and not ok[sp["pole+"]]  # a = 0 is not in front
    args = np.concatenate(ACOS_ARGS) if ACOS_ARGS else np.zeros(0, F)
    if model != "ortho":
        assert len(args) > 1000 and float(np.abs(args).max()) <= 0.7072  # the conditioning the header claims
        assert np.array_equal(bits(np_acos(args)), bits(orc.portable_acos(args))), "the test's own acos is not the oracle's portable_acos"


def test_acos_equals_the_oracle_over_its_whole_domain(orc):
    x = np.concatenate([np.linspace(-1.0, 1.0, 200001), [-1.5, 1.5, -0.5, 0.5, 0.0, -0.0]]).astype(F)
    assert np.array_equal(bits(np_acos(x)), bits(orc.portable_acos(x)))


# ---- the round trip ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("model", MODELS)
def test_round_trip_through_the_rays(pkg, model, size):
    """Every pixel-centre ray of rtu_sensor_rays, followed to t = 0.5, 3 and 40 and projected through the same sensor, comes back to
    (x, y) within 1/64 pixel: about ten roundings of 2^-24 on a coordinate of at most 256 pixels, times the conditioning factor 8 of
    the rows kept (sin(pol) >= 1/8), is 2e-3. Measured over these cases: at most 2.3e-5 pixel from (x, y) and 1.8e-5 from the float64
    evaluation with arctan2 of the same inputs (both orthographic 64 x 32, t = 40; equirect 1.5e-5 and 6.0e-6, fisheye 7.6e-6 and
    4.1e-6)."""
    W, H = size
    d = make(pkg, model, W, H, fov_deg=170.0)
    rays, _ = pkg.sensor_rays(d)
    y, x = np.divmod(np.arange(W * H), W)
    keep = np.ones(W * H, bool)
    if model == "fisheye":
        keep = (rays["dir"] != 0).any(axis=1)
    elif model == "equirect":
        keep = np.sin((y + 0.5) / H * math.pi) >= 1 / 8
    assert keep.sum() >= (0.35 if model == "fisheye" else 0.7) * W * H  # (the image circle of a 64 x 32 fisheye is 39 % of it)
    worst, worst64 = 0.0, 0.0
    for t in (0.5, 3.0, 40.0):
        P = (rays["org"] + rays["dir"] * F(t)).astype(F)
        fxfy, ok = pkg.sensor_project(d, P)
        assert ok[keep].all()
        dev = np.abs(fxfy[keep].astype(np.float64) - np.stack([x, y], 1)[keep]).max()
        fx64, fy64 = project64(d, P)
        dev64 = max(np.abs(fxfy[keep, 0] - fx64[keep]).max(), np.abs(fxfy[keep, 1] - fy64[keep]).max())
        worst, worst64 = max(worst, dev), max(worst64, dev64)
        assert dev <= 1 / 64, "%s t = %g: %g pixel from the pixel centre" % (model, t, dev)
    print("round trip %s %dx%d: at most %.3g pixel from (x, y), %.3g from the float64 arctan2 evaluation" % (model, W, H, worst, worst64))
    assert worst64 <= 1 / 64


# ---- the restatement of the accumulator ----------------------------------------------------------------------------------------------
def same_sensor(a, b):
    keys = ["pos", "right", "up", "forward"]
    if (a.model, a.width, a.height) != (b.model, b.width, b.height):
        return False
    if not all(np.array_equal(bits(v3(getattr(a, k))), bits(v3(getattr(b, k)))) for k in keys):
        return False
    if a.model == 1 and bits(F(a.fov_deg)) != bits(F(b.fov_deg)):
        return False
    return a.model != 2 or np.array_equal(bits(v3(a.extent)), bits(v3(b.extent)))


def lum(e):
    return (F(0.2126) * e[..., 0] + F(0.7152) * e[..., 1]) + F(0.0722) * e[..., 2]


def np_temporal_sensor(prev, cur, rgbz, hits, albedo, hist_prev, desc, moments=False, wrap=True):
    """The rules of "Temporal accumulation" with the lookup of "Temporal accumulation for sensors": (rgbz_out [H, W, 4], history
    [3 or 4, H, W, 4], info). wrap=False: the equirectangular columns do not wrap (what the seam test must tell apart)."""
    H, W = rgbz.shape[:2]
    c = rgbz[..., :3]
    valid = (hits["flags"].reshape(H, W) & RTU_RAY_HIT) != 0
    a = albedo.reshape(H, W, 4)[..., :3]
    d = np.where(a > F(0.01), a, F(1.0))
    Np, Pp = hits["N"].reshape(H, W, 3), hits["p"].reshape(H, W, 3)
    t, node = hits["t"].reshape(H, W), hits["node"].reshape(H, W)
    normal_min, maxh = F(desc.normal_min), F(desc.max_history)
    acc, nacc, wsum = np.zeros((H, W, 3), F), np.zeros((H, W), F), np.zeros((H, W), F)
    m1acc, m2acc = np.zeros((H, W), F), np.zeros((H, W), F)
    yg, xg = np.mgrid[0:H, 0:W]
    info = {"lookup": "none", "straddle": np.zeros((H, W), bool), "looked": np.zeros((H, W), bool)}
    with np.errstate(all="ignore"):
        e_cur = c / d
        plane_max = F(desc.sigma_plane) * t

        def tap(qx, qy, w, mask):
            nonlocal acc, nacc, wsum, m1acc, m2acc
            if wrap and prev.model == 0:
                qx = np.where(qx < 0, qx + W, np.where(qx >= W, qx - W, qx))
            inside = mask & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            Eq, Pq, Nq = hist_prev[0][cy, cx], hist_prev[1][cy, cx], hist_prev[2][cy, cx]
            ok = inside & (Eq[..., 3] > 0) & (np.ascontiguousarray(Nq[..., 3]).view(np.int32) == node)
            ok &= dot3(Np, Nq[..., :3]) >= normal_min
            ok &= np.abs(dot3(Np, Pq[..., :3] - Pp)) <= plane_max
            acc = np.where(ok[..., None], acc + Eq[..., :3] * w[..., None], acc)
            nacc = np.where(ok, nacc + Eq[..., 3] * w, nacc)
            wsum = np.where(ok, wsum + w, wsum)
            if moments:
                Mq = hist_prev[3][cy, cx]
                m1acc = np.where(ok, m1acc + Mq[..., 0] * w, m1acc)
                m2acc = np.where(ok, m2acc + Mq[..., 1] * w, m2acc)
        comparable = hist_prev is not None and (prev.model, prev.width, prev.height) == (cur.model, cur.width, cur.height)
        if not comparable:
            pass
        elif same_sensor(prev, cur):
            info["lookup"] = "static"
            tap(xg, yg, np.ones((H, W), F), valid)
        else:
            info["lookup"] = "reproject"
            fx, fy, ok = np_project(prev, Pp)
            looked = valid & ok & (fx >= F(-1.0)) & (fx < F(W)) & (fy >= F(-1.0)) & (fy < F(H))
            flx, fly = np.floor(np.where(looked, fx, F(0))), np.floor(np.where(looked, fy, F(0)))
            x0, y0 = flx.astype(int), fly.astype(int)
            wx, wy = fx - flx, fy - fly
            ux, uy = F(1.0) - wx, F(1.0) - wy
            tap(x0, y0, ux * uy, looked)
            tap(x0 + 1, y0, wx * uy, looked)
            tap(x0, y0 + 1, ux * wy, looked)
            tap(x0 + 1, y0 + 1, wx * wy, looked)
            info["looked"] = looked
            info["x0"] = x0
            info["straddle"] = looked & ((x0 < 0) | (x0 + 1 >= W))
        has = wsum > F(0.01)
        e_prev = np.where(has[..., None], acc / wsum[..., None], F(0.0))
        n_prev = np.where(has, nacc / wsum, F(0.0))
        m1_prev, m2_prev = np.where(has, m1acc / wsum, F(0.0)), np.where(has, m2acc / wsum, F(0.0))
        fin = np.isfinite(c).all(axis=-1)
        n_b = np.where(maxh < n_prev + F(1.0), maxh, n_prev + F(1.0))
        A = F(1.0) / n_b
        e_b = e_prev + (e_cur - e_prev) * A[..., None]
        fresh = n_prev == 0
        e = np.where(~fin[..., None], e_prev, np.where(fresh[..., None], e_cur, e_b))
        n = np.where(~fin, n_prev, np.where(fresh, F(1.0), n_b))
        keep = valid & (fin | ~fresh)
        out = rgbz.copy()
        out[..., :3] = np.where(keep[..., None], e * d, c)
        hist = np.zeros((4 if moments else 3, H, W, 4), F)
        if moments:
            l = lum(e_cur)
            l2 = l * l
            usable = fin & np.isfinite(l2)
            m1 = np.where(~usable, m1_prev, np.where(fresh, l, m1_prev + (l - m1_prev) * A))
            m2 = np.where(~usable, m2_prev, np.where(fresh, l2, m2_prev + (l2 - m2_prev) * A))
            hist[3][..., 0] = np.where(keep, m1, F(0.0))
            hist[3][..., 1] = np.where(keep, m2, F(0.0))
    hist[0][..., :3] = np.where(keep[..., None], e, F(0.0))
    hist[0][..., 3] = np.where(keep, n, F(0.0))
    hist[1][..., :3] = np.where(valid[..., None], Pp, F(0.0))
    hist[1][..., 3] = np.where(valid, t, F(0.0))
    hist[2][..., :3] = np.where(valid[..., None], Np, F(0.0))
    hist[2][..., 3] = np.where(valid, node, -1).astype(np.int32).view(F)
    assert out.dtype == F and e.dtype == F and n.dtype == F
    info["accepted"] = int((valid & has).sum())
    return out, hist, info


def chain_sensors(pkg, model, W, H):
    """Five sensors looking at the synthetic surfaces of make_inputs (around z = -5 .. -8, |x| <= 0.05 W, |y| <= 0.05 H): an equal
    pair (STATIC), a yaw, a translation, another field of view / window. up is -y: image rows grow with y, as the surfaces' do. The
    panorama looks AWAY from them, so they lie on its seam (and, a few degrees wide, on a few of its columns only: its lookups are
    tested on real guides by the yaw test below)."""
    def s(pos=(0.0, 0.0, 0.0), yaw=0.0, fov=70.0, ext=1.1):
        cy, sy = math.cos(yaw), math.sin(yaw)
        sign = 1.0 if model == "equirect" else -1.0
        right, fwd = (sign * -cy, 0.0, sign * -sy), (sign * -sy, 0.0, sign * cy)
        return pkg.sensor_desc(model, W, H, pos, right, (0.0, -1.0, 0.0), fwd, samples=1, fov_deg=fov, extent=(0.1 * W * ext, 0.1 * H * ext))
    return [s(), s(), s(yaw=0.013), s(pos=(0.23, -0.11, 0.4), yaw=0.013), s(fov=64.0, ext=1.25)]


def run_chain(sensors, frames, desc, form):
    res, hist = [], None
    for k in range(FRAMES):
        r = form(sensors[k - 1] if k else None, sensors[k], *frames[k], hist, desc)
        hist = r[1]
        res.append(r)
    return res


@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
@pytest.mark.parametrize("size", [(33, 17), (40, 30), (67, 35)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("model", MODELS)
def test_accumulators_equal_the_restatement(pkg, model, size, moments):
    W, H = size
    sensors = chain_sensors(pkg, model, W, H)
    for s in sensors:
        assert pkg.hip.rtu_sensor_rays(ctypes.byref(s), 0, 0, 0, None, None) == pkg.RTU_OK, "the test's sensor is outside the rules"
    frames = chain_inputs(pkg, W, H, 777 + W)
    for over in ({"max_history": 3}, {"sigma_plane": 0.4, "normal_min": -1.0}):
        desc = pkg.temporal_desc(W, H, **over)
        got = run_chain(sensors, frames, desc, lambda p, c, r, h, a, hp, d: pkg.temporal_accumulate_sensor(p, c, r, h, a, hp, d, moments=moments))
        want = run_chain(sensors, frames, desc, lambda p, c, r, h, a, hp, d: np_temporal_sensor(p, c, r, h, a, hp, d, moments=moments))
        assert [w[2]["lookup"] for w in want] == ["none", "static", "reproject", "reproject", "reproject"]
        for k in range(FRAMES):
            for what, g, w in (("image", got[k][0], want[k][0]), ("history", got[k][1], want[k][1])):
                diff = bits(g) != bits(w)
                assert not diff.any(), "%s %s frame %d %s: %d words differ, first at %s" % (model, over, k, what, diff.sum(), np.argwhere(diff)[0])
            invalid = ((frames[k][1]["flags"] & RTU_RAY_HIT) == 0).reshape(H, W)
            assert np.array_equal(bits(got[k][0])[invalid], bits(frames[k][0])[invalid]), "an invalid pixel was changed"
            if k >= 2 and model != "equirect":
                assert want[k][2]["accepted"] > 0.2 * (~invalid).sum(), "the chain's lookups find too little: %s" % want[k][2]["accepted"]
            if k >= 2 and model == "equirect" and "normal_min" in over:
                assert want[k][2]["accepted"] > 20, "the chain's lookups find too little: %s" % want[k][2]["accepted"]
        if model == "equirect":
            assert sum(int(want[k][2]["straddle"].sum()) for k in range(2, FRAMES)) > 20, "no lookup of the chain straddles the seam"
            nowrap = np_temporal_sensor(sensors[1], sensors[2], *frames[2], got[1][1], desc, moments=moments, wrap=False)
            assert (bits(nowrap[1]) != bits(got[2][1])).any(), "the restatement without the wrap gives the same bits: the wrap is not tested"


def test_sensors_of_another_model_take_no_history(pkg):
    W, H = 33, 17
    frames = chain_inputs(pkg, W, H, 3)
    desc = pkg.temporal_desc(W, H)
    a, b = chain_sensors(pkg, "fisheye", W, H)[2], chain_sensors(pkg, "ortho", W, H)[3]
    for moments in (False, True):
        _, h0 = pkg.temporal_accumulate_sensor(None, a, *frames[0], None, desc, moments=moments)
        fresh = pkg.temporal_accumulate_sensor(None, b, *frames[1], None, desc, moments=moments)
        other = pkg.temporal_accumulate_sensor(a, b, *frames[1], h0, desc, moments=moments)
        assert np.array_equal(bits(fresh[0]), bits(other[0])) and np.array_equal(bits(fresh[1]), bits(other[1]))


# ---- the STATIC path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_equal_sensors_give_the_camera_forms_bits(pkg, model):
    """Equal sensors: the one tap is the pixel itself, so a chain is the running mean — and it is the bits the camera forms give for
    equal cameras on the same arrays (the moments form with an all-STATIC table)."""
    W, H = 67, 35
    sensors = [chain_sensors(pkg, model, W, H)[0] for _ in range(FRAMES)]
    cams = [make_camera(pkg, W, H) for _ in range(FRAMES)]
    frames = chain_inputs(pkg, W, H, 99)
    first = frames[0]
    frames = [(f[0], first[1], first[2]) for f in frames]  # the same guides every frame
    desc = pkg.temporal_desc(W, H)
    motion = np.zeros(3, pkg.motion_dtype())
    motion["m"] = np.eye(3, 4, dtype=F)
    motion["g"] = np.eye(3, dtype=F)
    motion["flags"] = pkg.RTU_MOTION_STATIC
    for moments in (False, True):
        got = run_chain(sensors, frames, desc, lambda p, c, r, h, a, hp, d: pkg.temporal_accumulate_sensor(p, c, r, h, a, hp, d, moments=moments))
        if moments:
            cam = run_chain(cams, frames, desc, lambda p, c, r, h, a, hp, d: pkg.temporal_accumulate_moments(p, c, r, h, a, motion, hp, d))
        else:
            cam = run_chain(cams, frames, desc, lambda p, c, r, h, a, hp, d: pkg.temporal_accumulate(p, c, r, h, a, hp, d))
        for k in range(FRAMES):
            assert np.array_equal(bits(got[k][0]), bits(cam[k][0])) and np.array_equal(bits(got[k][1]), bits(cam[k][1])), (model, moments, k)
        valid = ((first[1]["flags"] & RTU_RAY_HIT) != 0).reshape(H, W)
        ok = valid & np.all([np.isfinite(f[0][..., :3]).all(-1) for f in frames], axis=0) & ~np.isnan(first[1]["N"]).any(-1).reshape(H, W)
        ok &= (first[1]["N"] != 0).any(-1).reshape(H, W)
        assert ok.sum() > 1000 and (got[-1][1][0][..., 3][ok] == FRAMES).all()
        mean = np.zeros((H, W, 3), F)  # the running mean, as the blend computes it
        d = np.where(first[2].reshape(H, W, 4)[..., :3] > F(0.01), first[2].reshape(H, W, 4)[..., :3], F(1.0))
        for k in range(FRAMES):
            with np.errstate(all="ignore"):  # (samples that are not finite: their pixels are not in `ok`)
                e = frames[k][0][..., :3] / d
                mean = e if k == 0 else mean + (e - mean) * (F(1.0) / F(k + 1))
        assert np.array_equal(bits(got[-1][1][0][..., :3][ok]), bits(mean[ok]))


# ---- a pure yaw of a panorama on the oracle's guides -----------------------------------------------------------------------------------
YAW_W, YAW_H = 64, 32


def yawed(pkg, basis, columns, samples=0):
    """The equirect 64 x 32 sensor at `basis` turned about its up axis by `columns` columns (2 pi columns / 64; float64, rounded)."""
    pos, right, up, fwd = (np.array(v, np.float64) for v in basis)
    a = 2 * math.pi * columns / YAW_W
    r2, f2 = right * math.cos(a) + fwd * math.sin(a), fwd * math.cos(a) - right * math.sin(a)
    return pkg.sensor_desc("equirect", YAW_W, YAW_H, pos, r2, up, f2, samples=samples)


def interior_pixels(hits):
    """Hit pixels whose 3 x 3 neighbourhood — columns wrapped, rows inside the image — hits the same node."""
    node = np.where((hits["flags"] & RTU_RAY_HIT) != 0, hits["node"], -1).reshape(YAW_H, YAW_W)
    ok = node >= 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            sh = np.roll(node, (dy, dx), axis=(0, 1))
            ok &= sh == node
    ok[0], ok[-1] = False, False
    return ok


@pytest.fixture(scope="module")
def yaw_guides(pkg, orc, golden):
    """Per step (5 and 5.5 columns a frame): the sensors of seven frames and their guides from the oracle (albedo ones)."""
    scene = golden("p11simple_200x150").scene(pkg)
    basis = camera_basis(scene)
    out = {}
    for step in (5.0, 5.5):
        sensors = [yawed(pkg, basis, step * k) for k in range(7)]
        guides = []
        for s in sensors:
            rays, _ = pkg.sensor_rays(s)
            hits = orc.trace_rays(scene, rays, threads=4).astype(pkg.hit_dtype())
            guides.append(hits)
        out[step] = (sensors, guides)
    return out


def yaw_run(pkg, sensors, guides, form):
    rng = np.random.default_rng(5)
    albedo = np.ones((YAW_W * YAW_H, 4), F)
    hist, res = None, []
    for k, (s, hits) in enumerate(zip(sensors, guides)):
        rgbz = rng.random((YAW_H, YAW_W, 4), dtype=F)
        r = form(sensors[k - 1] if k else None, s, rgbz, hits, albedo, hist, pkg.temporal_desc(YAW_W, YAW_H))
        hist = r[1]
        res.append(r)
    return res


def test_a_pure_yaw_is_followed_across_the_seam(pkg, yaw_guides):
    """A yaw by whole columns maps every pixel centre onto a pixel centre of the previous panorama — across the seam too —, so the
    history of an interior pixel grows by one a frame: after frame k, n >= k + 0.5 on every interior hit pixel but at most 0.5 %.
    Measured: no interior pixel falls short at 5 columns a frame (0 of 836 per frame), nor at 5.5 (0 of 836 .. 839).

    What the wrap changes cannot be seen in n at all: the projection answers lon in [0, 2 pi], fx in [-0.5, width - 0.5], so a lookup at
    the seam always keeps the taps of one column with a weight of at least one half, and n_prev = nacc / wsum is normalised by the
    accepted weight (measured: the restatement without the wrap passes the n check too, 0 short at either step). Without the wrap
    such a pixel takes its colour from ONE column where it lies between two. So the wrap is shown on
    the colours: at 5.5 columns a frame the restatement WITHOUT the wrap must differ from the host form, at pixels whose taps straddle
    the seam and only there, while the restatement with it is the host form bit for bit."""
    for step in (5.0, 5.5):
        sensors, guides = yaw_guides[step]
        got = yaw_run(pkg, sensors, guides, lambda *a: pkg.temporal_accumulate_sensor(*a))
        want = yaw_run(pkg, sensors, guides, np_temporal_sensor)
        for k in range(1, 7):
            assert np.array_equal(bits(got[k][0]), bits(want[k][0])) and np.array_equal(bits(got[k][1]), bits(want[k][1])), (step, k)
            inner = interior_pixels(guides[k])
            n = got[k][1][0][..., 3]
            short = inner & ~(n >= k + 0.5)
            seam = inner & want[k][2]["straddle"]
            print("yaw %.1f frame %d: %d interior pixels, %d short, %d of them with taps across the seam" % (step, k, inner.sum(), short.sum(), seam.sum()))
            assert inner.sum() > 800
            assert short.sum() <= 0.005 * inner.sum(), "yaw %.1f frame %d: %d of %d interior pixels fall short" % (step, k, short.sum(), inner.sum())
            assert want[k][2]["looked"][inner].all()
            crossed = inner & (np.abs(want[k][2]["x0"] - np.mgrid[0:YAW_H, 0:YAW_W][1]) > YAW_W // 2)
            assert crossed.sum() >= 20, "no interior pixel's history came across the seam"
    sensors, guides = yaw_guides[5.5]
    got = yaw_run(pkg, sensors, guides, lambda *a: pkg.temporal_accumulate_sensor(*a))
    differing = 0
    for k in range(1, 7):
        prev_hist = got[k - 1][1]
        rng = np.random.default_rng(5)
        rgbz = [rng.random((YAW_H, YAW_W, 4), dtype=F) for _ in range(k + 1)][k]
        albedo = np.ones((YAW_W * YAW_H, 4), F)
        desc = pkg.temporal_desc(YAW_W, YAW_H)
        nowrap = np_temporal_sensor(sensors[k - 1], sensors[k], rgbz, guides[k], albedo, prev_hist, desc, wrap=False)
        withwrap = np_temporal_sensor(sensors[k - 1], sensors[k], rgbz, guides[k], albedo, prev_hist, desc)
        assert np.array_equal(bits(withwrap[1]), bits(got[k][1]))
        diff = (bits(nowrap[1][0]) != bits(got[k][1][0])).any(axis=-1)
        assert not (diff & ~withwrap[2]["straddle"]).any(), "the wrap changed a pixel away from the seam"
        differing += int((diff & interior_pixels(guides[k])).sum())
    assert differing >= 6, "without the wrap nothing changes at the seam columns: the test does not see the wrap (%d)" % differing


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
def test_in_place_and_refusals(pkg, moments):
    W, H = 33, 17
    planes = 4 if moments else 3
    fn = pkg.hip.rtu_temporal_accumulate_sensor_moments if moments else pkg.hip.rtu_temporal_accumulate_sensor
    sensors = chain_sensors(pkg, "fisheye", W, H)
    frames = chain_inputs(pkg, W, H, 5)
    d = pkg.temporal_desc(W, H)
    res = run_chain(sensors, frames, d, lambda p, c, r, h, a, hp, dd: pkg.temporal_accumulate_sensor(p, c, r, h, a, hp, dd, moments=moments))
    rgbz, hits, albedo = frames[3]
    prev_hist = np.ascontiguousarray(res[2][1])
    buf, hist = rgbz.copy(), np.empty((planes, H, W, 4), F)

    def call(desc=d, prev=sensors[2], cur=sensors[3], a=None, hp=prev_hist.ctypes.data, ho=None, out=None):
        a = a or [buf.ctypes.data, hits.ctypes.data, albedo.ctypes.data]
        return fn(ctypes.byref(desc) if desc is not None else None, ctypes.byref(prev) if prev is not None else None,
                  ctypes.byref(cur) if cur is not None else None, a[0], a[1], a[2], hp, ho if ho is not None else hist.ctypes.data,
                  out if out is not None else buf.ctypes.data)
    assert call() == pkg.RTU_OK                       # rgbz_out == rgbz
    assert np.array_equal(bits(buf), bits(res[3][0])) and np.array_equal(bits(hist), bits(res[3][1]))
    buf[:] = rgbz
    assert call(ho=prev_hist.ctypes.data) == pkg.RTU_ERR_ARG          # aliased histories: the same buffer, and any overlap
    big = np.zeros(2 * prev_hist.size, F)
    big[:prev_hist.size] = prev_hist.reshape(-1)
    assert call(hp=big.ctypes.data, ho=big.ctypes.data + 16) == pkg.RTU_ERR_ARG
    assert call(hp=big.ctypes.data, ho=big.ctypes.data + 4 * prev_hist.size) == pkg.RTU_OK
    for bad in ({"max_history": 0}, {"max_history": 65536}, {"sigma_plane": 0.0}, {"sigma_plane": float("nan")}, {"normal_min": 1.5},
                {"normal_min": float("nan")}, {"flags": 2}, {"width": 0}, {"height": -1}, {"width": W - 1}):
        bd = pkg.temporal_desc(W, H)
        for k, v in bad.items():
            setattr(bd, k, v)
        assert call(desc=bd) == pkg.RTU_ERR_ARG, bad
    bd = pkg.temporal_desc(W, H)
    bd.reserved[1] = 1
    assert call(desc=bd) == pkg.RTU_ERR_ARG
    assert call(desc=None) == pkg.RTU_ERR_ARG and call(cur=None) == pkg.RTU_ERR_ARG and call(prev=None) == pkg.RTU_ERR_ARG
    assert call(prev=None, hp=None) == pkg.RTU_OK     # no history: no previous sensor needed
    # a current sensor of another size is refused; a previous one of another size or model is another image: no lookup, RTU_OK
    assert call(cur=chain_sensors(pkg, "fisheye", W + 1, H)[3]) == pkg.RTU_ERR_ARG
    buf[:] = rgbz
    assert call(prev=chain_sensors(pkg, "fisheye", W + 1, H)[2]) == pkg.RTU_OK
    fresh = pkg.temporal_accumulate_sensor(None, sensors[3], rgbz, hits, albedo, None, d, moments=moments)
    assert np.array_equal(bits(hist), bits(fresh[1]))
    buf[:] = rgbz
    for field, value in (("model", 3), ("fov_deg", 0.0), ("fov_deg", 361.0), ("samples", -1), ("flags", 4), ("max_bounce", 99)):
        for which in ("prev", "cur"):
            s = chain_sensors(pkg, "fisheye", W, H)[2 if which == "prev" else 3]
            setattr(s, field, value)
            assert call(**{which: s}) == pkg.RTU_ERR_ARG, (field, which)
    s = chain_sensors(pkg, "fisheye", W, H)[3]
    s.right[0] = 2.0                                  # no orthonormal frame
    assert call(cur=s) == pkg.RTU_ERR_ARG
    s = chain_sensors(pkg, "fisheye", W, H)[3]
    s.pos[1] = float("inf")
    assert call(cur=s) == pkg.RTU_ERR_ARG
    s = chain_sensors(pkg, "ortho", W, H)[3]
    s.extent[0] = 0.0
    assert call(cur=s, prev=None, hp=None) == pkg.RTU_ERR_ARG
    args = [buf.ctypes.data, hits.ctypes.data, albedo.ctypes.data]
    for k in range(3):
        assert call(a=[None if j == k else x for j, x in enumerate(args)]) == pkg.RTU_ERR_ARG
    assert fn(ctypes.byref(d), ctypes.byref(sensors[2]), ctypes.byref(sensors[3]), *args, None, None, buf.ctypes.data) == pkg.RTU_ERR_ARG
    assert fn(ctypes.byref(d), ctypes.byref(sensors[2]), ctypes.byref(sensors[3]), *args, None, hist.ctypes.data, None) == pkg.RTU_ERR_ARG


def test_projection_refusals(pkg):
    d = make(pkg, "equirect", 8, 4)
    P, out, ok = np.zeros((2, 3), F), np.zeros((2, 2), F), np.zeros(2, np.uint8)
    fn = pkg.hip.rtu_sensor_project
    assert fn(ctypes.byref(d), P.ctypes.data, 2, out.ctypes.data, ok.ctypes.data) == pkg.RTU_OK
    assert fn(ctypes.byref(d), None, 0, None, None) == pkg.RTU_OK
    assert fn(None, P.ctypes.data, 2, out.ctypes.data, ok.ctypes.data) == pkg.RTU_ERR_ARG
    for k in range(3):
        a = [P.ctypes.data, out.ctypes.data, ok.ctypes.data]
        a[k] = None
        assert fn(ctypes.byref(d), a[0], 2, a[1], a[2]) == pkg.RTU_ERR_ARG
    d.model = 7
    assert fn(ctypes.byref(d), P.ctypes.data, 2, out.ctypes.data, ok.ctypes.data) == pkg.RTU_ERR_ARG
    with pytest.raises(pkg.RtuError):
        pkg.sensor_project(d, P)
