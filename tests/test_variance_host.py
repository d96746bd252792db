"""The host forms of variance-guided filtering (rtu_temporal_accumulate_moments, rtu_variance, rtu_denoise_variance; include/rtu_render.h
"Variance-guided filtering") — the executable statements of the rules, which the device forms must reproduce bit for bit
(tests/test_gpu_variance.py) — against the existing accumulator, against independent numpy restatements with shifted views, and their
effect on the oracle's own path-traced samples. No GPU."""
import ctypes

import numpy as np
import pytest

from test_denoise_host import K, RTU_RAY_INVALID, SIZES, bits, dot3, inputs_ok, make_inputs, oracle_guides
from test_temporal_host import CHAINS, FRAMES, ORBIT_FRAMES, chain_cameras, chain_inputs, make_camera, orbit_scene
from test_temporal_motion_host import CASES, case_cameras, table

F = np.float32
RTU_RAY_HIT = 1
K3 = [F(0.25), F(0.5), F(0.25)]
EPS = F(1e-8)


def lum(e):
    return (F(0.2126) * e[..., 0] + F(0.7152) * e[..., 1]) + F(0.0722) * e[..., 2]


def demod(albedo, H, W):
    a = albedo.reshape(H, W, 4)[..., :3]
    return np.where(a > F(0.01), a, F(1.0))


def moments_chain(pkg, cams, frames, desc, motion, cap):
    """[(image, history [4, H, W, 4])] of rtu_temporal_accumulate_moments along a chain."""
    res, hist = [], None
    for k in range(len(frames)):
        out, hist = pkg.temporal_accumulate_moments(cams[k - 1] if k else None, cams[k], *frames[k], motion, hist, desc, cap)
        res.append((out, hist))
    return res


def motion_chain(pkg, cams, frames, desc, motion, cap):
    res, hist = [], None
    for k in range(len(frames)):
        out, hist = pkg.temporal_accumulate_motion(cams[k - 1] if k else None, cams[k], *frames[k], motion, hist, desc, cap)
        res.append((out, hist))
    return res


def luminance_frames(frames, H, W):
    """The frames with the image {l, l * l, 0, z} and albedo {1, 1, 1, 0}: what the existing accumulator turns into the moments."""
    out = []
    for rgbz, hits, albedo in frames:
        with np.errstate(all="ignore"):
            l = lum(rgbz[..., :3] / demod(albedo, H, W))
            img = np.stack([l, l * l, np.zeros_like(l), rgbz[..., 3]], axis=-1).astype(F)
        alb = np.zeros_like(albedo)
        alb[:, :3] = 1.0
        out.append((img, hits, alb))
    return out


def all_chains(pkg, W, H):
    """(what, cameras, frames, temporal desc, table, history_cap): the chains of test_temporal_host with an all-static table and the
    cases of test_temporal_motion_host."""
    for ci, (name, over) in enumerate(CHAINS):
        yield "chain %s %s" % (name, over), chain_cameras(pkg, W, H)[name], chain_inputs(pkg, W, H, 4321 + ci), pkg.temporal_desc(W, H, **over), table("static"), 0
    for ci, (kind, n, camname, cap, over) in enumerate(CASES):
        yield ("table %s[%d] cameras %s cap %d %s" % (kind, n, camname, cap, over), case_cameras(pkg, W, H, camname), chain_inputs(pkg, W, H, 1234 + ci),
               pkg.temporal_desc(W, H, **over), table(kind)[:n], cap)


# ---- 1. the moments against the existing accumulator -------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_moments_against_the_existing_accumulator(pkg, size):
    W, H = size
    blended = 0
    for what, cams, frames, desc, motion, cap in all_chains(pkg, W, H):
        got = moments_chain(pkg, cams, frames, desc, motion, cap)
        want = motion_chain(pkg, cams, frames, desc, motion, cap)
        lframes = luminance_frames(frames, H, W)
        for (rgbz, _, _), (img, _, _) in zip(frames, lframes):  # the condition of the comparison: finite in the same pixels
            assert np.array_equal(np.isfinite(rgbz[..., :3]).all(-1), np.isfinite(img[..., :3]).all(-1))
        alt = motion_chain(pkg, cams, lframes, desc, motion, cap)
        for k in range(FRAMES):
            assert np.array_equal(bits(got[k][0]), bits(want[k][0])), "%s frame %d: the image" % (what, k)
            assert np.array_equal(bits(got[k][1][:3]), bits(want[k][1])), "%s frame %d: the planes E, P, N" % (what, k)
            M = got[k][1][3]
            diff = bits(M[..., :2]) != bits(alt[k][1][0][..., :2])
            assert not diff.any(), "%s frame %d: %d words of M differ, first at %s" % (what, k, diff.sum(), np.argwhere(diff)[0])
            assert not bits(M[..., 2:]).any(), "M.zw is zero"
            assert np.array_equal(bits(got[k][1][0][..., 3]), bits(alt[k][1][0][..., 3])), "the two chains count the same history"
            blended += int((got[k][1][0][..., 3] > 1).sum())
    assert size == (1, 1) or blended > 0


def test_moments_skip_a_sample_whose_square_overflows(pkg):
    """The stated rule: c finite but l * l not (here l = 1e20 / d): E and n take the sample, M keeps what it had — zeros when fresh."""
    W, H = 7, 5
    cams = [make_camera(pkg, W, H) for _ in range(3)]
    rgbz, hits, albedo = make_inputs(pkg, W, H, 77)
    hits["node"] = np.where((hits["flags"] & RTU_RAY_HIT) != 0, 1, -1)
    vi = np.flatnonzero((hits["flags"] & RTU_RAY_HIT) != 0)
    vi = [i for i in vi if not np.isnan(hits["N"][i]).any() and (hits["N"][i] != 0).any()]
    a, b = vi[0], vi[1]
    f0, f1, f2 = rgbz.copy(), rgbz.copy(), rgbz.copy()
    f0.reshape(-1, 4)[a, :3] = 1e20   # fresh and overflowing
    f1.reshape(-1, 4)[b, :3] = 1e20   # overflowing on top of one sample
    frames = [(f, hits, albedo) for f in (f0, f1, f2)]
    desc, motion = pkg.temporal_desc(W, H), table("static")
    got = moments_chain(pkg, cams, frames, desc, motion, 0)
    want = motion_chain(pkg, cams, frames, desc, motion, 0)
    for k in range(3):
        assert np.array_equal(bits(got[k][0]), bits(want[k][0])) and np.array_equal(bits(got[k][1][:3]), bits(want[k][1]))
    E0, M0, E1, M1, M2 = (x.reshape(-1, 4) for x in (got[0][1][0], got[0][1][3], got[1][1][0], got[1][1][3], got[2][1][3]))
    assert E0[a, 3] == 1 and np.isfinite(E0[a, :3]).all() and not bits(M0[a]).any()
    assert E1[b, 3] == 2 and np.isfinite(E1[b, :3]).all() and np.array_equal(bits(M1[b]), bits(M0[b])) and M0[b, 0] > 0
    assert np.isfinite(got[2][1][3]).all() and got[2][1][0].reshape(-1, 4)[b, 3] == 3 and M2[b, 0] > 0


# ---- 2. the numpy restatements --------------------------------------------------------------------------------------------------
def shifted(H, W, dy, dx, s):
    y0, y1, x0, x1 = max(0, -dy * s), min(H, H - dy * s), max(0, -dx * s), min(W, W - dx * s)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s))


def guide_weight(N, P, rp, ps, qs, nlog2):
    dot = dot3(N[ps], N[qs])
    t = np.where(dot > 0, dot, F(0.0))
    for _ in range(nlog2):
        t = t * t
    x = dot3(N[ps], P[qs] - P[ps]) * rp[ps]
    return t * (F(1.0) / (F(1.0) + x * x))


def np_variance(hist, hits, desc):
    """Rule 2 of "Variance-guided filtering" restated: (v [H, W], counts of the branches)."""
    H, W = hist.shape[1:3]
    n, m1, m2 = hist[0][..., 3], hist[3][..., 0], hist[3][..., 1]
    live = ((hits["flags"].reshape(H, W) & RTU_RAY_HIT) != 0) & (n > 0)
    N, P, t = hits["N"].reshape(H, W, 3), hits["p"].reshape(H, W, 3), hits["t"].reshape(H, W)
    mh = F(desc.min_history)
    with np.errstate(all="ignore"):
        x = m2 - m1 * m1
        vt = np.where(x > 0, x, F(0.0))
        rp = F(1.0) / (F(desc.sigma_plane) * t)
        s1, s2, ws = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                sl = shifted(H, W, dy, dx, 1)
                if sl is None:
                    continue
                ps, qs = sl
                w = guide_weight(N, P, rp, ps, qs, desc.normal_log2_power)
                m = live[qs]
                s1[ps] = np.where(m, s1[ps] + m1[qs] * w, s1[ps])
                s2[ps] = np.where(m, s2[ps] + m2[qs] * w, s2[ps])
                ws[ps] = np.where(m, ws[ps] + w, ws[ps])
        has = ws > 0
        a1, a2 = s1 / ws, s2 / ws
        x = a2 - a1 * a1
        vs = np.where(has & (x > 0), x, F(0.0))
        short = live & (n < mh)
        var = np.where(short, np.where(vs > vt, vs, vt) * (mh / n), vt)
        v = np.where(live, var / n, F(0.0))
    assert v.dtype == F
    return v, {"short_with_taps": int((short & has).sum()), "short_without_taps": int((short & ~has).sum()), "long": int((live & ~short).sum()),
               "spatial_wins": int((short & (vs > vt)).sum())}


def np_denoise_variance(rgbz, hits, albedo, v, desc):
    """Rule 3 restated: (output [H, W, 4], number of (pixel, pass) pairs that fell back to e_p)."""
    H, W = rgbz.shape[:2]
    c = rgbz[..., :3]
    valid = (hits["flags"].reshape(H, W) & RTU_RAY_HIT) != 0
    d = demod(albedo, H, W)
    N, P = hits["N"].reshape(H, W, 3), hits["p"].reshape(H, W, 3)
    fallbacks = 0
    with np.errstate(all="ignore"):
        rp = F(1.0) / (F(desc.sigma_plane) * hits["t"].reshape(H, W))
        sl2 = F(desc.sigma_lum) * F(desc.sigma_lum)
        e, vv = c / d, np.array(v, F).reshape(H, W)
        for i in range(desc.n_passes):
            s = 1 << i
            g, ks = np.zeros((H, W), F), np.zeros((H, W), F)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    sl = shifted(H, W, dy, dx, 1)
                    if sl is None:
                        continue
                    ps, qs = sl
                    k = K3[dy + 1] * K3[dx + 1]
                    g[ps] = np.where(valid[qs], g[ps] + vv[qs] * k, g[ps])
                    ks[ps] = np.where(valid[qs], ks[ps] + k, ks[ps])
            r = F(1.0) / (sl2 * (g / ks) + EPS)
            l = lum(e)
            acc, vacc, wsum = np.zeros((H, W, 3), F), np.zeros((H, W), F), np.zeros((H, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    sl = shifted(H, W, dy, dx, s)
                    if sl is None:
                        continue
                    ps, qs = sl
                    tw = guide_weight(N, P, rp, ps, qs, desc.normal_log2_power)
                    dl = l[qs] - l[ps]
                    wc = F(1.0) / (F(1.0) + (dl * dl) * r[ps])
                    w = ((K[dy + 2] * K[dx + 2]) * tw) * wc
                    assert w.dtype == F
                    m = valid[qs]
                    acc[ps] = np.where(m[..., None], acc[ps] + e[qs] * w[..., None], acc[ps])
                    vacc[ps] = np.where(m, vacc[ps] + vv[qs] * (w * w), vacc[ps])
                    wsum[ps] = np.where(m, wsum[ps] + w, wsum[ps])
            upd = valid & (wsum > 0)
            fallbacks += int((valid & ~upd).sum())
            ws2 = wsum * wsum
            e = np.where(upd[..., None], acc / wsum[..., None], e)
            vv = np.where(upd & (ws2 > 0), vacc / ws2, vv)
        out = rgbz.copy()
        out[..., :3] = np.where(valid[..., None], e * d, c)
    assert out.dtype == F
    return out, fallbacks


def make_variance(W, H, seed):
    """A variance image: log-uniform over twelve decades, with zeros, denormals and 1e30 among them."""
    rng = np.random.default_rng(seed)
    v = (F(10.0) ** rng.uniform(-9, 3, (H, W))).astype(F)
    pick = rng.random((H, W))
    v[pick < 0.15] = 0.0
    v[(pick >= 0.15) & (pick < 0.2)] = np.array([0x00000123], np.uint32).view(F)[0]
    v[(pick >= 0.2) & (pick < 0.25)] = 1e30
    if W * H > 1:
        v.reshape(-1)[:3] = [0.0, np.array([1], np.uint32).view(F)[0], 1e30]
    return v


@pytest.fixture(scope="module")
def cases(pkg):
    """(W, H) -> (rgbz, hits, albedo, v) of section 22's inputs and make_variance, and a moments history with its frame's hits; made
    once and left unchanged."""
    out = {}
    for k, (W, H) in enumerate(SIZES):
        rgbz, hits, albedo = make_inputs(pkg, W, H, 1234 + k)
        inputs_ok(rgbz, hits, albedo)
        v = make_variance(W, H, 99 + k)
        frames = chain_inputs(pkg, W, H, 4321)
        hist = moments_chain(pkg, chain_cameras(pkg, W, H)["X"], frames, pkg.temporal_desc(W, H), table("static"), 0)[-1][1]
        out[(W, H)] = (rgbz, hits, albedo, v, hist, frames[-1][1])
        for a in out[(W, H)]:
            a.setflags(write=False)
    v = out[(67, 35)][3]
    assert (v == 0).any() and (v == 1e30).any() and ((v > 0) & (v < np.finfo(F).tiny)).any()
    return out


VARIANCE_SETS = ({}, {"min_history": 2, "sigma_plane": 0.2, "normal_log2_power": 0}, {"min_history": 100, "normal_log2_power": 7})
FILTER_SETS = ({}, {"sigma_lum": 0.35, "sigma_plane": 0.2, "normal_log2_power": 0}, {"sigma_lum": 8.0, "normal_log2_power": 7})


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_variance_equals_the_numpy_restatement(pkg, cases, size):
    hist, hits = cases[size][4:]
    for over in VARIANCE_SETS:
        desc = pkg.variance_desc(size[0], size[1], **over)
        got = pkg.variance(hist, hits, desc)
        want, counts = np_variance(hist, hits, desc)
        diff = bits(got) != bits(want)
        assert not diff.any(), "%s: %d words differ, first at %s" % (over, diff.sum(), np.argwhere(diff)[0])
        print(size, over, counts)
        # ---- 3. both branches, and the short one with and without a usable tap
        if size == (67, 35) and not over:
            for key in ("short_with_taps", "short_without_taps", "long", "spatial_wins"):
                assert counts[key] > 0, "no pixel took the branch %r: %s" % (key, counts)
        invalid = ((hits["flags"] & RTU_RAY_HIT) == 0).reshape(size[1], size[0])
        assert not bits(got)[invalid].any() and (got >= 0).all()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_filter_equals_the_numpy_restatement(pkg, cases, size):
    rgbz, hits, albedo, v = cases[size][:4]
    changed = fallbacks = 0
    for n_passes in range(1, 7):  # steps 1 .. 32: beyond 7 x 5 from the fourth pass, beyond 35 rows at the sixth
        for over in FILTER_SETS:
            desc = pkg.variance_desc(size[0], size[1], n_passes=n_passes, **over)
            got = pkg.denoise_variance(rgbz, hits, albedo, v, desc)
            want, fb = np_denoise_variance(rgbz, hits, albedo, v, desc)
            diff = bits(got) != bits(want)
            assert not diff.any(), "%d passes %s: %d words differ, first at %s" % (n_passes, over, diff.sum(), np.argwhere(diff)[0])
            changed += int((bits(got) != bits(rgbz)).sum())
            fallbacks += fb
    if size != (1, 1):
        assert changed > 0, "the filter changed nothing"
        assert fallbacks > 0, "no pixel fell back to its own value (wsum == 0)"


def test_the_variance_steers_the_filter(pkg, cases):
    """What the feature is: with a large variance the filter is the guide-only blur, with none a pixel all but keeps its colour. The
    factor: with v = 0, r = 1 / 1e-8, so a tap whose luminance differs by more than 1e-3 weighs less than 1 / (1 + 1e-6 * 1e8) < 0.01 of
    what it weighs in the blur, and the 24 of them together (their h sum to 0.86 against the centre's 0.14) move the pixel by less than
    0.01 * 0.86 / 0.14 = 0.06 of a typical difference; taps closer than 1e-3 in luminance are a thousandth of the taps of this noise."""
    rgbz, hits, albedo = cases[(67, 35)][:3]
    valid = ((hits["flags"] & RTU_RAY_HIT) != 0).reshape(35, 67) & np.isfinite(rgbz[..., :3]).all(-1)
    zero = pkg.denoise_variance(rgbz, hits, albedo, np.zeros((35, 67), F))
    big = pkg.denoise_variance(rgbz, hits, albedo, np.full((35, 67), 1e6, F))
    moved = lambda out: np.abs(out[..., :3][valid] - rgbz[..., :3][valid]).mean()
    assert moved(zero) < 0.1 * moved(big)


# ---- 4. pass-through, in place, refusals -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES[1:], ids=lambda s: "%dx%d" % s)
def test_invalid_pixels_and_z_pass_through(pkg, cases, size):
    rgbz, hits, albedo, v = cases[size][:4]
    invalid = ((hits["flags"] & RTU_RAY_HIT) == 0).reshape(size[1], size[0])
    assert invalid.any() and (hits["flags"] == RTU_RAY_INVALID).any() and (hits["flags"] == 0).any()
    assert np.isnan(rgbz[invalid][:, :3]).any() and np.isnan(rgbz[..., 3]).any(), "no odd bit patterns to carry through"
    for n_passes in (1, 3, 5):
        out = pkg.denoise_variance(rgbz, hits, albedo, v, pkg.variance_desc(n_passes=n_passes))
        assert np.array_equal(bits(out)[invalid], bits(rgbz)[invalid])
        assert np.array_equal(bits(out[..., 3]), bits(rgbz[..., 3]))
        assert (bits(out)[~invalid][:, :3] != bits(rgbz)[~invalid][:, :3]).any()


def test_in_place_and_defaults(pkg, cases):
    rgbz, hits, albedo, v, hist, hhits = cases[(67, 35)]
    d = pkg.variance_desc()
    assert (d.n_passes, d.sigma_lum, d.normal_log2_power, d.min_history, ctypes.sizeof(d)) == (3, 2.0, 5, 4, 40) and d.sigma_plane == F(0.05)
    want = pkg.denoise_variance(rgbz, hits, albedo, v)
    buf = rgbz.copy()
    d.width, d.height = 67, 35
    assert pkg.hip.rtu_denoise_variance(ctypes.byref(d), buf.ctypes.data, hits.ctypes.data, albedo.ctypes.data, v.ctypes.data, buf.ctypes.data) == pkg.RTU_OK
    assert np.array_equal(bits(buf), bits(want))
    # the accumulator in place, as the motion form
    W, H = 67, 35
    cams, frames = chain_cameras(pkg, W, H)["X"], chain_inputs(pkg, W, H, 5)
    td, motion = pkg.temporal_desc(W, H), table("static")
    res = moments_chain(pkg, cams, frames, td, motion, 0)
    buf, out_hist, prev = frames[3][0].copy(), np.empty((4, H, W, 4), F), np.ascontiguousarray(res[2][1])

    def acc(hp=prev.ctypes.data, ho=None, desc=td, cap=0, mo=motion.ctypes.data):
        return pkg.hip.rtu_temporal_accumulate_moments(ctypes.byref(desc), ctypes.byref(cams[2]), ctypes.byref(cams[3]), buf.ctypes.data,
                                                       frames[3][1].ctypes.data, frames[3][2].ctypes.data, hp, ho if ho is not None else out_hist.ctypes.data,
                                                       buf.ctypes.data, mo, 3, cap)
    assert acc() == pkg.RTU_OK
    assert np.array_equal(bits(buf), bits(res[3][0])) and np.array_equal(bits(out_hist), bits(res[3][1]))
    buf[:] = frames[3][0]
    assert acc(ho=prev.ctypes.data) == pkg.RTU_ERR_ARG
    big = np.zeros(2 * prev.size, F)
    big[:prev.size] = prev.reshape(-1)
    assert acc(hp=big.ctypes.data, ho=big.ctypes.data + 4 * prev.size - 16) == pkg.RTU_ERR_ARG  # the last pixel of M overlaps
    assert acc(hp=big.ctypes.data, ho=big.ctypes.data + 4 * prev.size) == pkg.RTU_OK
    assert acc(cap=-1) == pkg.RTU_ERR_ARG and acc(cap=65536) == pkg.RTU_ERR_ARG and acc(mo=None) == pkg.RTU_ERR_ARG
    assert acc(desc=pkg.temporal_desc(W, H, flags=2)) == pkg.RTU_ERR_ARG and acc(desc=pkg.temporal_desc(W, H, max_history=0)) == pkg.RTU_ERR_ARG
    bad = motion.copy()
    bad["reserved"][1][0] = 1
    assert acc(mo=bad.ctypes.data) == pkg.RTU_ERR_ARG


def test_argument_errors(pkg, cases):
    rgbz, hits, albedo, v, hist, hhits = cases[(7, 5)]
    for bad in ({"n_passes": 0}, {"n_passes": 9}, {"sigma_lum": 0.0}, {"sigma_plane": -1.0}, {"sigma_lum": float("nan")}, {"sigma_plane": float("nan")},
                {"normal_log2_power": -1}, {"normal_log2_power": 8}, {"min_history": 0}, {"min_history": 65536}):
        with pytest.raises(pkg.RtuError):
            pkg.denoise_variance(rgbz, hits, albedo, v, pkg.variance_desc(**bad))
        with pytest.raises(pkg.RtuError):
            pkg.variance(hist, hhits, pkg.variance_desc(**bad))
    for k in range(3):
        d = pkg.variance_desc(7, 5)
        d.reserved[k] = 1
        with pytest.raises(pkg.RtuError):
            pkg.denoise_variance(rgbz, hits, albedo, v, d)
        with pytest.raises(pkg.RtuError):
            pkg.variance(hist, hhits, d)
    d = pkg.variance_desc(7, 5)
    args = [rgbz.ctypes.data, hits.ctypes.data, albedo.ctypes.data, v.ctypes.data, np.empty_like(rgbz).ctypes.data]
    for k in range(5):
        assert pkg.hip.rtu_denoise_variance(ctypes.byref(d), *[None if j == k else a for j, a in enumerate(args)]) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_denoise_variance(None, *args) == pkg.RTU_ERR_ARG
    vargs = [hist.ctypes.data, hhits.ctypes.data, np.empty((5, 7), F).ctypes.data]
    for k in range(3):
        assert pkg.hip.rtu_variance(ctypes.byref(d), *[None if j == k else a for j, a in enumerate(vargs)]) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_variance(None, *vargs) == pkg.RTU_ERR_ARG and pkg.hip.rtu_variance_defaults(None) == pkg.RTU_ERR_ARG
    for k, bad in (("width", 0), ("height", -1), ("width", 65537)):
        d = pkg.variance_desc(7, 5)
        setattr(d, k, bad)
        assert pkg.hip.rtu_denoise_variance(ctypes.byref(d), *args) == pkg.RTU_ERR_ARG and pkg.hip.rtu_variance(ctypes.byref(d), *vargs) == pkg.RTU_ERR_ARG


# ---- 5. quality, on the oracle alone ----------------------------------------------------------------------------------------------
REST_FRAMES = 16


def accumulate_on_the_oracle(pkg, orc, golden, tag, orbit):
    """The last of ORBIT_FRAMES frames along the orbit of test_temporal_host (orbit) or of REST_FRAMES frames of the golden camera at
    rest, one sample of S = 16 each, accumulated with the moments: (raw last sample, accumulated image, history, hits, albedo, 256 spp)."""
    g = golden(tag)
    scene = g.scene(pkg)
    W, H = g.width, g.height
    desc = pkg.temporal_desc(W, H)
    motion = table("static", scene.desc.n_nodes)
    centre = oracle_guides(pkg, orc, scene, W, H)[0][(H // 2) * W + W // 2]
    hist = prev = None
    for k in range(ORBIT_FRAMES if orbit else REST_FRAMES):
        s = orbit_scene(pkg, scene, k, float(centre["t"])) if orbit else scene
        frame = pkg.frame_setup(s.desc.camera, W, H, samples=16, gather_bounces=4)
        sample = orc.sample_images(s, W, H, 16, k, 1, gi=True, threads=8)[0]
        if orbit or k == 0:
            hits, albedo = oracle_guides(pkg, orc, s, W, H)
        assert ((hits["flags"] & RTU_RAY_HIT) != 0).all(), "a closed room: every pixel hits"
        out, hist = pkg.temporal_accumulate_moments(prev, frame, sample, hits, albedo, motion, hist, desc)
        prev = frame
    ref = orc.render_paths(s, W, H, 256, threads=8)[0]
    return sample, out, hist, hits, albedo, ref


def quality_row(pkg, data, vdesc=None):
    """RMSE over all pixels, linear rgb, against 256 spp, divided by the raw last sample's: accumulated; rtu_denoise with its defaults
    and with the new filter's pass count; the new filter."""
    sample, out, hist, hits, albedo, ref = data
    vdesc = vdesc if vdesc is not None else pkg.variance_desc()

    def rmse(img):
        return float(np.sqrt(np.mean((img[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)) ** 2)))
    raw = rmse(sample)
    v = pkg.variance(hist, hits, vdesc)
    return {"raw": raw, "acc": rmse(out) / raw, "fixed5": rmse(pkg.denoise(out, hits, albedo)) / raw,
            "fixedN": rmse(pkg.denoise(out, hits, albedo, pkg.denoise_desc(n_passes=vdesc.n_passes))) / raw,
            "new": rmse(pkg.denoise_variance(out, hits, albedo, v, vdesc)) / raw}


# Measured ratios of the new filter with its defaults (the rows are in DESIGN.md section 25); each bound is the ratio times 1.25,
# rounded up to two digits. p13's 256-spp reference is itself full of fireflies: it gets a bound and no ordering claim.
#   p11 orbit 0.123 (accumulated 0.287, fixed filter 0.212 at 5 passes and 0.143 at 3)
#   p11 at rest 0.105 (0.251, 0.210, 0.138)        p13 at rest 0.167 (0.270, 0.145, 0.141)
QUALITY = [("p11_p2_120x68", True, 0.16, True), ("p11_p2_120x68", False, 0.14, True), ("p13_p2_96x72", False, 0.21, False)]


@pytest.mark.parametrize("tag,orbit,bound,ordered", QUALITY, ids=["p11-orbit", "p11-rest", "p13-rest"])
def test_quality_on_the_oracle(pkg, orc, golden, tag, orbit, bound, ordered):
    data = accumulate_on_the_oracle(pkg, orc, golden, tag, orbit)
    n = data[2][0][..., 3]
    print("%s %s: %.1f %% of the pixels have n >= 2, mean n %.2f" % (tag, "orbit" if orbit else "rest", 100 * (n >= 2).mean(), n.mean()))
    if orbit:
        assert (n >= 2).mean() >= 0.8, "the orbit's step is too large for this test: a condition on its input"
    row = quality_row(pkg, data)
    print("%s %s: RMSE raw %.5f; ratios: accumulated %.3f, fixed filter 5 passes %.3f, fixed filter %d passes %.3f, variance-guided %.3f"
          % (tag, "orbit" if orbit else "rest", row["raw"], row["acc"], row["fixed5"], pkg.variance_desc().n_passes, row["fixedN"], row["new"]))
    if ordered:
        assert row["new"] < row["fixed5"] and row["new"] < row["fixedN"], "the variance-guided filter is not better than the fixed one: %s" % row
    assert row["new"] < bound, "variance-guided: RMSE ratio %.3f" % row["new"]
