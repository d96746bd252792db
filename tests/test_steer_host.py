"""The host forms of steered sampling (rtu_sample_allocation, rtu_extra_sample_rays, rtu_temporal_refine; include/rtu_render.h
"Steered sampling") — the executable statements of the rules, which the device forms must reproduce bit for bit
(tests/test_gpu_steer.py) — against independent numpy restatements, against rtu_camera_sample_rays and the one-tap accumulator, and
their effect on the oracle's own path-traced samples. No GPU."""
import ctypes

import numpy as np
import pytest

from test_denoise_host import SIZES, bits, oracle_guides
from test_temporal_host import ORBIT_FRAMES, chain_cameras, chain_inputs, make_camera, orbit_scene
from test_temporal_motion_host import table
from test_variance_host import REST_FRAMES, accumulate_on_the_oracle, cases, demod, lum, make_variance, moments_chain  # noqa: F401 (cases: a fixture)

F = np.float32
U = np.uint32
RTU_RAY_HIT = 1
BUDGETS = ("0", "1", "quarter", "pixels", "four")
EXTRAS = (1, 3, 15)


def budget_of(name, pixels):
    return {"0": 0, "1": 1, "quarter": pixels // 4, "pixels": pixels, "four": 4 * pixels}[name]


def mix32(x):
    x = np.array(x, U)
    with np.errstate(over="ignore"):
        x = x ^ (x >> U(16))
        x = x * U(0x7feb352d)
        x = x ^ (x >> U(15))
        x = x * U(0x846ca68b)
        x = x ^ (x >> U(16))
    return x


def np_weights(hist, hits, v):
    H, W = hist.shape[1:3]
    n, m1 = hist[0][..., 3], hist[3][..., 0]
    live = ((hits["flags"].reshape(H, W) & RTU_RAY_HIT) != 0) & (n > 0)
    with np.errstate(all="ignore"):
        x = (np.array(v, F).reshape(H, W) / (m1 * m1 + F(1.0))) * F(16777216.0)
    assert x.dtype == F
    pos = live & (x > 0)  # (a NaN fails)
    small = pos & (x < F(1048576.0))
    w = np.zeros((H, W), np.uint64)
    w[small] = x[small].astype(np.uint64)  # truncation
    w[pos & ~small] = 1048576
    return w, live


def np_allocation(hist, hits, v, budget, E, k):
    """Rule 1 of "Steered sampling" restated in integer arithmetic: (counts, offsets, total, what happened)."""
    H, W = hist.shape[1:3]
    w, live = np_weights(hist, hits, v)
    w = w.reshape(-1)
    wsum = int(w.sum(dtype=np.uint64))
    assert wsum < 1 << 46
    pix = np.arange(H * W, dtype=np.uint64)
    if wsum == 0:
        z = np.zeros((H, W), U)
        return z, z.copy(), 0, {"up": 0, "clamped": 0, "cut": 0}
    with np.errstate(over="ignore"):
        h = (mix32((pix.astype(U) + U(0x9e3779b9) * U((k + 1) & 0xffffffff))) >> U(16)).astype(np.uint64)
    raw = (np.uint64(budget) * w + ((h * np.uint64(wsum)) >> np.uint64(16))) // np.uint64(wsum)
    floor = (np.uint64(budget) * w) // np.uint64(wsum)
    c = np.minimum(raw, np.uint64(E))
    o = np.cumsum(c) - c
    offs = np.minimum(o, np.uint64(budget))
    cnt = np.minimum(c, np.uint64(budget) - offs)
    what = {"up": int((raw > floor).sum()), "clamped": int((raw > E).sum()), "cut": int((cnt < c).sum())}
    return cnt.astype(U).reshape(H, W), offs.astype(U).reshape(H, W), min(int(c.sum()), budget), what


def steer_history(cases, size):
    """Section 25's test history of this size and the hits of its frame, with some valid pixels' E zeroed (n == 0: no history)."""
    hist, hits = (np.array(a) for a in cases[size][4:])
    valid = np.flatnonzero((hits["flags"] & RTU_RAY_HIT) != 0)
    if size != (1, 1):
        hist[0].reshape(-1, 4)[valid[1::7]] = 0.0
    return hist, hits


def odd_variance(W, H, seed):
    """make_variance (zeros, denormals, 1e30 among twelve decades) with NaNs added."""
    v = make_variance(W, H, seed).copy()
    if W * H > 1:
        v.reshape(-1)[5::11] = np.nan
    return v


# ---- 1. the allocation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_allocation_equals_the_integer_restatement(pkg, cases, size):
    W, H = size
    hist, hits = steer_history(cases, size)
    seen = {"up": 0, "clamped": 0, "cut": 0}
    for vname, v in (("variance()", pkg.variance(hist, hits)), ("odd", odd_variance(W, H, 7)), ("1e30", np.full((H, W), 1e30, F))):
        w, live = np_weights(hist, hits, v)
        assert not w[~live].any()
        for bname in BUDGETS:
            for E in EXTRAS:
                for k in (0, 1, 0xffffffff):
                    budget = budget_of(bname, W * H)
                    desc = pkg.steer_desc(W, H, budget=budget, max_extra=E, frame_index=k)
                    counts, offsets, total = pkg.sample_allocation(hist, hits, v, desc)
                    wc, wo, wt, what = np_allocation(hist, hits, v, budget, E, k)
                    assert np.array_equal(counts, wc) and np.array_equal(offsets, wo) and total == wt, (vname, bname, E, k)
                    assert total <= budget and counts.max() <= E and total == int(counts.sum(dtype=np.uint64))
                    assert np.array_equal(offsets.reshape(-1), (np.cumsum(counts.reshape(-1), dtype=np.uint64) - counts.reshape(-1)).astype(U))
                    assert not counts[~live].any()
                    for key in seen:
                        seen[key] += what[key]
    print(size, seen)
    if size != (1, 1):
        invalid = (hits["flags"] & RTU_RAY_HIT) == 0
        fresh = ~invalid & (hist[0].reshape(-1, 4)[:, 3] == 0)
        assert invalid.any() and fresh.any(), "no invalid pixel / no valid pixel without history"
        assert seen["up"] > 0, "no pixel was rounded up by the dither"
        assert seen["clamped"] > 0, "no pixel was clamped at max_extra"
        assert seen["cut"] > 0, "no pixel was cut at the budget"


def test_allocation_without_weight_and_odd_variances(pkg, cases):
    W, H = 67, 35
    hist, hits = steer_history(cases, (W, H))
    for v in (np.zeros((H, W), F), np.full((H, W), np.nan, F), np.full((H, W), -1.0, F), np.full((H, W), np.array([1], U).view(F)[0], F)):
        counts, offsets, total = pkg.sample_allocation(hist, hits, v, pkg.steer_desc(budget=W * H, max_extra=15))
        assert total == 0 and not counts.any() and not offsets.any(), "Wsum == 0 gives no ray"
    v = odd_variance(W, H, 3)
    w, live = np_weights(hist, hits, v)
    assert (v[live] == 0).any() and np.isnan(v[live]).any() and (v[live] == 1e30).any() and ((v[live] > 0) & (v[live] < np.finfo(F).tiny)).any()
    assert not w[live & ~(v > 0)].any() and (w[live & (v == 1e30)] == 1048576).all() and ((w > 0) & (w < 1048576)).any()
    # the dither spends a budget below one ray per pixel, and moves it from frame to frame
    a = pkg.sample_allocation(hist, hits, v, pkg.steer_desc(budget=W * H // 4, max_extra=3, frame_index=0))
    b = pkg.sample_allocation(hist, hits, v, pkg.steer_desc(budget=W * H // 4, max_extra=3, frame_index=1))
    assert a[2] >= 0.5 * (W * H // 4) and b[2] >= 0.5 * (W * H // 4) and not np.array_equal(a[0], b[0])


# ---- 2. the extra rays ------------------------------------------------------------------------------------------------------------
def lens_camera(pkg, W, H, S):
    f = make_camera(pkg, W, H, shift=(0.1, -0.2), yaw=0.01)
    f.samples, f.dof = S, 0.05
    f.lens_up[:] = [0.0, 1.0, 0.0]
    f.lens_right[:] = [1.0, 0.0, 0.0]
    return f


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_extra_rays_are_camera_sample_rays_gathered_by_owner(pkg, cases, size):
    W, H = size
    hist, hits = steer_history(cases, size)
    v = pkg.variance(hist, hits)
    used = set()
    for S, E, k in ((1, 1, 0), (4, 3, 0), (4, 3, 6), (16, 15, 21), (4096, 15, 4100)):
        frame = lens_camera(pkg, W, H, S)
        desc = pkg.steer_desc(W, H, budget=2 * W * H, max_extra=E, frame_index=k)
        counts, offsets, total = pkg.sample_allocation(hist, hits, v, desc)
        rays, keys, owner = pkg.extra_sample_rays(frame, counts, offsets, desc)
        assert len(rays) == total
        big = lens_camera(pkg, W, H, S * (1 + E))
        want_owner = np.repeat(np.arange(W * H, dtype=U), counts.reshape(-1))
        assert np.array_equal(owner, want_owner)
        j = np.arange(total) - offsets.reshape(-1)[owner] if total else np.zeros(0, int)
        for jj in range(E):
            sample = S + (k % S) * E + jj
            assert S <= sample < S * (1 + E)
            used.add((S, E, k % S, jj, sample))
            sel = j == jj
            if not sel.any():
                continue
            r, ky = pkg.camera_sample_rays(big, sample)
            assert rays[sel].tobytes() == r[owner[sel]].tobytes() and np.array_equal(keys[sel], ky[owner[sel]]), (S, E, k, jj)
        if size != (1, 1):
            assert total > 0
    # distinct over (k mod S, j) for a given S and E
    for S, E in ((4, 3),):
        idx = [S + km * E + j for km in range(S) for j in range(E)]
        assert len(set(idx)) == len(idx) and min(idx) == S and max(idx) == S * (1 + E) - 1


def test_extra_rays_refusals(pkg, cases):
    W, H = 7, 5
    hist, hits = steer_history(cases, (W, H))
    desc = pkg.steer_desc(W, H, budget=W * H, max_extra=3)
    counts, offsets, total = pkg.sample_allocation(hist, hits, pkg.variance(hist, hits), desc)
    assert total > 0
    frame = lens_camera(pkg, W, H, 4)
    with pytest.raises(pkg.RtuError):
        pkg.extra_sample_rays(frame, counts, offsets, desc, capacity=total - 1)
    with pytest.raises(pkg.RtuError):
        pkg.extra_sample_rays(frame, counts + U(4), offsets, desc, capacity=10 * W * H)
    with pytest.raises(pkg.RtuError):
        pkg.extra_sample_rays(lens_camera(pkg, W, H, 0), counts, offsets, desc)
    with pytest.raises(pkg.RtuError):
        pkg.extra_sample_rays(lens_camera(pkg, W, H, 16385), counts, offsets, desc)  # 16385 * 4 > 65536
    pkg.extra_sample_rays(lens_camera(pkg, W, H, 16384), counts, offsets, desc)
    d = pkg.steer_desc(W, H + 1, budget=W * H, max_extra=3)
    rays = np.zeros(total, pkg.ray_dtype())
    keys, owner = np.zeros(total, U), np.zeros(total, U)
    args = [counts.ctypes.data, offsets.ctypes.data, total, rays.ctypes.data, keys.ctypes.data, owner.ctypes.data]
    assert pkg.hip.rtu_extra_sample_rays(ctypes.byref(d), ctypes.byref(frame), *args) == pkg.RTU_ERR_ARG  # another size
    assert pkg.hip.rtu_extra_sample_rays(ctypes.byref(desc), ctypes.byref(frame), *args) == pkg.RTU_OK
    assert pkg.hip.rtu_extra_sample_rays(None, ctypes.byref(frame), *args) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_extra_sample_rays(ctypes.byref(desc), None, *args) == pkg.RTU_ERR_ARG
    for i in (0, 1, 3, 4, 5):
        assert pkg.hip.rtu_extra_sample_rays(ctypes.byref(desc), ctypes.byref(frame), *[None if j == i else a for j, a in enumerate(args)]) == pkg.RTU_ERR_ARG


# ---- 3. the fold ------------------------------------------------------------------------------------------------------------------
def np_refine(hist, rgbz, hits, albedo, counts, offsets, rgbt, max_history):
    """Rule 3 restated in numpy float32: (rgbz, hist)."""
    H, W = hist.shape[1:3]
    hist, rgbz = hist.copy(), rgbz.copy()
    E, M = hist[0], hist[3]
    live = ((hits["flags"].reshape(H, W) & RTU_RAY_HIT) != 0) & (E[..., 3] > 0) & (counts > 0)
    d = demod(albedo, H, W)
    e, n, m1, m2 = E[..., :3].copy(), E[..., 3].copy(), M[..., 0].copy(), M[..., 1].copy()
    rgbt = np.concatenate([np.array(rgbt, F).reshape(-1, 4), np.zeros((1, 4), F)])
    with np.errstate(all="ignore"):
        for j in range(int(counts.max()) if counts.size else 0):
            has = live & (counts > j)
            c = rgbt[np.where(has, offsets + U(j), len(rgbt) - 1)][..., :3]
            take = has & np.isfinite(c).all(-1)
            e_cur = c / d
            n1 = np.minimum(n + F(1.0), F(max_history))
            a = F(1.0) / n1
            e1 = e + (e_cur - e) * a[..., None]
            l = lum(e_cur)
            l2 = l * l
            mom = take & np.isfinite(l2)
            m1 = np.where(mom, m1 + (l - m1) * a, m1)
            m2 = np.where(mom, m2 + (l2 - m2) * a, m2)
            e = np.where(take[..., None], e1, e)
            n = np.where(take, n1, n)
        assert e.dtype == F and n.dtype == F and m1.dtype == F
        E[..., :3] = np.where(live[..., None], e, E[..., :3])
        E[..., 3] = np.where(live, n, E[..., 3])
        M[..., 0] = np.where(live, m1, M[..., 0])
        M[..., 1] = np.where(live, m2, M[..., 1])
        rgbz[..., :3] = np.where(live[..., None], e * d, rgbz[..., :3])
    return rgbz, hist


def fold_inputs(pkg, cases, size, seed, budget_name="four", E=15):
    """A history with the image, hits and albedo of its frame, an allocation, and samples with NaN, infinite and overflowing ones."""
    W, H = size
    frames = chain_inputs(pkg, W, H, 4321)
    res = moments_chain(pkg, chain_cameras(pkg, W, H)["X"], frames, pkg.temporal_desc(W, H), table("static"), 0)
    rgbz, hist = res[-1]
    hits, albedo = frames[-1][1], frames[-1][2]
    assert np.array_equal(bits(hist), bits(cases[size][4])), "section 25's test history"
    hist = hist.copy()
    valid = np.flatnonzero((hits["flags"] & RTU_RAY_HIT) != 0)
    if size != (1, 1):
        hist[0].reshape(-1, 4)[valid[1::7]] = 0.0
    desc = pkg.steer_desc(W, H, budget=budget_of(budget_name, W * H), max_extra=E, frame_index=seed)
    counts, offsets, total = pkg.sample_allocation(hist, hits, pkg.variance(hist, hits), desc)
    rng = np.random.default_rng(seed)
    rgbt = rng.uniform(0.0, 2.0, (total, 4)).astype(F)
    if total > 8:
        rgbt[1, 0], rgbt[3, 2], rgbt[5, 1], rgbt[7, :3] = np.nan, np.inf, -np.inf, 1e20  # 1e20: finite, its luminance squared is not
    return hist, rgbz, hits, albedo, counts, offsets, rgbt


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_fold_equals_the_numpy_restatement(pkg, cases, size):
    W, H = size
    changed = 0
    for seed, bname, E, over in ((1, "four", 15, {}), (2, "pixels", 3, {"max_history": 3}), (3, "quarter", 1, {}), (4, "0", 3, {})):
        hist, rgbz, hits, albedo, counts, offsets, rgbt = fold_inputs(pkg, cases, size, seed, bname, E)
        td = pkg.temporal_desc(W, H, **over)
        got_img, got_hist = pkg.temporal_refine(hist, rgbz, hits, albedo, counts, offsets, rgbt, td)
        want_img, want_hist = np_refine(hist, rgbz, hits, albedo, counts, offsets, rgbt, td.max_history)
        for what, g, w in (("image", got_img, want_img), ("history", got_hist, want_hist)):
            diff = bits(g) != bits(w)
            assert not diff.any(), "%s %s: %d words differ, first at %s" % ((seed, bname, E), what, diff.sum(), np.argwhere(diff)[0])
        # P, N, z and every pixel that takes no sample pass bit for bit
        assert np.array_equal(bits(got_hist[1:3]), bits(hist[1:3])) and np.array_equal(bits(got_img[..., 3]), bits(rgbz[..., 3]))
        assert np.array_equal(bits(got_hist[3][..., 2:]), bits(hist[3][..., 2:]))
        idle = (counts == 0) | ((hits["flags"].reshape(H, W) & RTU_RAY_HIT) == 0) | ~(hist[0][..., 3] > 0)
        assert np.array_equal(bits(got_hist)[:, idle], bits(hist)[:, idle]) and np.array_equal(bits(got_img)[idle], bits(rgbz)[idle])
        changed += int((bits(got_hist) != bits(hist)).sum())
    assert size == (1, 1) or changed > 0


def test_fold_skips_what_the_accumulator_skips(pkg, cases):
    W, H = 67, 35
    hist, rgbz, hits, albedo, counts, offsets, rgbt = fold_inputs(pkg, cases, (W, H), 1)
    assert len(rgbt) > 8
    owner = np.repeat(np.arange(W * H), counts.reshape(-1))
    base = rgbt.copy()
    base[[1, 3, 5, 7], :3] = 0.5
    got = pkg.temporal_refine(hist, rgbz, hits, albedo, counts, offsets, rgbt)[1]
    ref = pkg.temporal_refine(hist, rgbz, hits, albedo, counts, offsets, base)[1]
    n_got, n_ref = got[0][..., 3].reshape(-1), ref[0][..., 3].reshape(-1)
    capped = n_ref == pkg.temporal_desc().max_history
    for p in set(owner[[1, 3, 5, 7]]):  # not finite: neither E nor n takes the sample; 1e20: E and n take it, the moments skip it
        assert capped[p] or abs(n_got[p] - (n_ref[p] - sum(owner[i] == p for i in (1, 3, 5)))) < 1e-4  # (n is not an integer after a reprojection)
    p = owner[7]
    assert np.isfinite(got[0].reshape(-1, 4)[p]).all() and np.isfinite(got[3].reshape(-1, 4)[p]).all() and got[0].reshape(-1, 4)[p, 0] > 1e10
    assert np.isfinite(got[0]).all() and np.isfinite(got[3]).all()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_one_extra_sample_is_a_second_accumulation_on_the_one_tap_path(pkg, cases, size):
    W, H = size
    frames = chain_inputs(pkg, W, H, 4321)
    cams = chain_cameras(pkg, W, H)["X"]
    td, motion = pkg.temporal_desc(W, H), table("static")
    rgbz, hist = moments_chain(pkg, cams, frames, td, motion, 0)[-1]
    _, hits, albedo = frames[-1]
    sample = chain_inputs(pkg, W, H, 999)[2][0].copy()  # other noise, with its own NaN and infinite samples
    sample[..., 3] = rgbz[..., 3]
    want_img, want_hist = pkg.temporal_accumulate_moments(cams[-1], cams[-1], sample, hits, albedo, motion, hist, td)
    counts = np.ones((H, W), U)
    offsets = np.arange(W * H, dtype=U).reshape(H, W)
    got_img, got_hist = pkg.temporal_refine(hist, rgbz, hits, albedo, counts, offsets, sample.reshape(-1, 4), td)
    # the pixels that take the sample in the fold and find their own history in the accumulator: valid, n > 0, a usable normal
    N = hits["N"].reshape(H, W, 3)
    with np.errstate(all="ignore"):
        own = ((N * N).sum(-1) >= td.normal_min)
    ok = ((hits["flags"].reshape(H, W) & RTU_RAY_HIT) != 0) & (hist[0][..., 3] > 0) & own
    assert size == (1, 1) or ok.sum() > 0.5 * W * H
    assert np.array_equal(bits(got_hist)[:, ok], bits(want_hist)[:, ok]) and np.array_equal(bits(got_img)[ok], bits(want_img)[ok])
    if size != (1, 1):
        assert (~np.isfinite(sample[..., :3]).all(-1) & ok).any(), "no sample that is not finite among the compared pixels"
        assert (bits(got_hist)[0][ok] != bits(hist)[0][ok]).any()


def test_fold_in_place_and_refusals(pkg, cases):
    W, H = 67, 35
    hist, rgbz, hits, albedo, counts, offsets, rgbt = fold_inputs(pkg, cases, (W, H), 5)
    want_img, want_hist = pkg.temporal_refine(hist, rgbz, hits, albedo, counts, offsets, rgbt)
    h, img = hist.copy(), rgbz.copy()
    td = pkg.temporal_desc(W, H)
    args = [h.ctypes.data, hits.ctypes.data, albedo.ctypes.data, counts.ctypes.data, offsets.ctypes.data, rgbt.ctypes.data, len(rgbt), img.ctypes.data]
    assert pkg.hip.rtu_temporal_refine(ctypes.byref(td), *args) == pkg.RTU_OK
    assert np.array_equal(bits(h), bits(want_hist)) and np.array_equal(bits(img), bits(want_img))
    h[:], img[:] = hist, rgbz
    for i in (0, 1, 2, 3, 4, 5, 7):
        assert pkg.hip.rtu_temporal_refine(ctypes.byref(td), *[None if j == i else a for j, a in enumerate(args)]) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_temporal_refine(None, *args) == pkg.RTU_ERR_ARG
    short = list(args)
    short[6] = len(rgbt) - 1
    assert pkg.hip.rtu_temporal_refine(ctypes.byref(td), *short) == pkg.RTU_ERR_ARG  # a sample outside rgbt
    for bad in ({"max_history": 0}, {"max_history": 65536}, {"sigma_plane": 0.0}, {"flags": 2}, {"width": 0}, {"height": 65537}):
        d = pkg.temporal_desc(W, H)
        for k2, val in bad.items():
            setattr(d, k2, val)
        assert pkg.hip.rtu_temporal_refine(ctypes.byref(d), *args) == pkg.RTU_ERR_ARG
    assert np.array_equal(bits(h), bits(hist)) and np.array_equal(bits(img), bits(rgbz)), "a refused call wrote"


def test_allocation_defaults_and_refusals(pkg, cases):
    W, H = 7, 5
    hist, hits = steer_history(cases, (W, H))
    v = pkg.variance(hist, hits)
    d = pkg.steer_desc()
    assert (d.width, d.height, d.budget, d.max_extra, d.frame_index, ctypes.sizeof(d)) == (0, 0, 0, 3, 0, 32)
    for bad in ({"max_extra": 0}, {"max_extra": 16}, {"max_extra": -1}, {"budget": (1 << 26) + 1}):
        with pytest.raises(pkg.RtuError):
            pkg.sample_allocation(hist, hits, v, pkg.steer_desc(**bad))
    pkg.sample_allocation(hist, hits, v, pkg.steer_desc(budget=1 << 26, max_extra=15, frame_index=0xffffffff))
    for k in range(3):
        d = pkg.steer_desc(W, H)
        d.reserved[k] = 1
        with pytest.raises(pkg.RtuError):
            pkg.sample_allocation(hist, hits, v, d)
    d = pkg.steer_desc(W, H, budget=9)
    counts, offsets, total = np.zeros((H, W), U), np.zeros((H, W), U), ctypes.c_uint32(0)
    args = [hist.ctypes.data, hits.ctypes.data, v.ctypes.data, counts.ctypes.data, offsets.ctypes.data, ctypes.addressof(total)]
    assert pkg.hip.rtu_sample_allocation(ctypes.byref(d), *args) == pkg.RTU_OK and total.value == int(counts.sum()) <= 9
    for i in range(6):
        assert pkg.hip.rtu_sample_allocation(ctypes.byref(d), *[None if j == i else a for j, a in enumerate(args)]) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_sample_allocation(None, *args) == pkg.RTU_ERR_ARG and pkg.hip.rtu_steer_defaults(None) == pkg.RTU_ERR_ARG
    for k, bad in (("width", 0), ("height", -1), ("width", 65537)):
        d = pkg.steer_desc(W, H)
        setattr(d, k, bad)
        assert pkg.hip.rtu_sample_allocation(ctypes.byref(d), *args) == pkg.RTU_ERR_ARG


# ---- 4. quality, on the oracle alone ----------------------------------------------------------------------------------------------
S_ORACLE, E_ORACLE = 16, 3


def steered_rows(pkg, orc, golden, tag, orbit):
    """After accumulate_on_the_oracle: the last frame's history refined with budget = pixels extra rays, max_extra 3, allocated by the
    variance (steered) and one per pixel (uniform); the extra samples are the oracle's sample images at S (1 + E) spp. RMSE over all
    pixels against 256 spp as ratios to the raw last sample's, before and after the variance-guided filter."""
    sample, out, hist, hits, albedo, ref = accumulate_on_the_oracle(pkg, orc, golden, tag, orbit)
    g = golden(tag)
    scene = g.scene(pkg)
    W, H = g.width, g.height
    k = (ORBIT_FRAMES if orbit else REST_FRAMES) - 1
    centre = oracle_guides(pkg, orc, scene, W, H)[0][(H // 2) * W + W // 2]
    s = orbit_scene(pkg, scene, k, float(centre["t"])) if orbit else scene
    first = S_ORACLE + (k % S_ORACLE) * E_ORACLE
    extra = orc.sample_images(s, W, H, S_ORACLE * (1 + E_ORACLE), first, E_ORACLE, gi=True, threads=8)
    extra = np.stack([np.asarray(x, F).reshape(H * W, 4) for x in extra])  # [j][pixel]
    vdesc = pkg.variance_desc()

    def rmse(img, mask=None):
        d = (img[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)) ** 2
        return float(np.sqrt(np.mean(d if mask is None else d[mask])))

    v = pkg.variance(hist, hits, vdesc)
    desc = pkg.steer_desc(W, H, budget=W * H, max_extra=E_ORACLE, frame_index=k)
    counts, offsets, total = pkg.sample_allocation(hist, hits, v, desc)
    uniform = (np.ones((H, W), U), np.arange(W * H, dtype=U).reshape(H, W), W * H)
    short = hist[0][..., 3] < vdesc.min_history
    rows = {"raw": rmse(sample), "total": total, "short": float(short.mean()), "max_count": int(counts.max())}
    raw, raw_short = rows["raw"], (rmse(sample, short) if short.any() else float("nan"))
    rows["acc"] = rmse(out) / raw
    rows["acc_filtered"] = rmse(pkg.denoise_variance(out, hits, albedo, v, vdesc)) / raw
    for name, (c, o, n) in (("steered", (counts, offsets, total)), ("uniform", uniform)):
        owner = np.repeat(np.arange(W * H), c.reshape(-1))
        j = np.arange(n) - o.reshape(-1)[owner]
        img, h2 = pkg.temporal_refine(hist, out, hits, albedo, c, o, extra[j, owner])
        flt = pkg.denoise_variance(img, hits, albedo, pkg.variance(h2, hits, vdesc), vdesc)
        rows[name] = rmse(img) / raw
        rows[name + "_filtered"] = rmse(flt) / raw
        if short.any():
            rows[name + "_short"] = rmse(img, short) / raw_short
            rows[name + "_filtered_short"] = rmse(flt, short) / raw_short
    return rows


# Measured ratios (the rows are in DESIGN.md section 26), before / after the filter; each bound is the steered ratio times 1.25, rounded
# up to two digits. budget = 8160 rays, max_extra 3: the steered allocation spends 7577 / 7506 of them (the clamp at max_extra).
#   p11 orbit: accumulated 0.2875 / 0.1235; uniform 0.2785 / 0.1184; steered 0.2745 / 0.1180
#              over the 0.2 % of the pixels with n < min_history: uniform 0.518 / 0.254; steered 0.349 / 0.221
#   p11 rest:  accumulated 0.2509 / 0.1054; uniform 0.2427 / 0.1034; steered 0.2411 / 0.1041 — AFTER THE FILTER STEERED IS NOT BELOW
#              UNIFORM, and no pixel has n < min_history to assert it over instead: that ordering is not asserted.
QUALITY = [(True, 0.35, 0.15, True), (False, 0.31, 0.14, False)]


@pytest.mark.parametrize("orbit,bound,bound_filtered,ordered_filtered", QUALITY, ids=["p11-orbit", "p11-rest"])
def test_quality_on_the_oracle(pkg, orc, golden, orbit, bound, bound_filtered, ordered_filtered):
    rows = steered_rows(pkg, orc, golden, "p11_p2_120x68", orbit)
    print("p11 %s: %s" % ("orbit" if orbit else "rest", {k: (round(x, 4) if isinstance(x, float) else x) for k, x in rows.items()}))
    assert rows["total"] >= 0.9 * 120 * 68, "the steered allocation spent %d of %d rays: a condition on its input" % (rows["total"], 120 * 68)
    assert rows["steered"] < rows["uniform"] < rows["acc"], "before the filter steered is not below uniform: %s" % rows
    if ordered_filtered:
        assert rows["steered_filtered"] < rows["uniform_filtered"] < rows["acc_filtered"], "after the filter steered is not below uniform: %s" % rows
    if orbit:
        assert rows["short"] > 0, "no pixel with n < min_history: a condition on the input"
        assert rows["steered_short"] < rows["uniform_short"] and rows["steered_filtered_short"] < rows["uniform_filtered_short"], rows
    assert rows["steered"] < bound and rows["steered_filtered"] < bound_filtered, rows
