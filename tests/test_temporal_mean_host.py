"""What the temporal accumulators compute AT REST, said independently in float64: a history at rest is the mean of what went into
it. No GPU. Every other arithmetic check of the accumulators is a transcription of the same rules in the same order (bit for bit)
or an RMSE bound on the oracle; this one is neither. It runs the host forms — rtu_temporal_accumulate, _motion, _moments, _gradient,
_sparse and rtu_temporal_refine of include/rtu_render.h, which tests/test_gpu_*.py hold the kernels to bit for bit — over K = 40
frames of one camera (every pixel takes the one-tap path) and compares with float64 means and recursions of the samples. The GPU
file tests/test_gpu_session_lifetimes.py runs the same chains through the device forms and applies the same checks.

THE TOLERANCE is derived, not tuned. One blend update of tp_pixel (raytracer-utah_amd/csrc/rtu_temporal.h) rounds SIX times per
channel: the demodulating divide e_cur = c / d, the subtraction e_cur - e_prev, the divide A = 1 / n that gives the weight, the
product (e_cur - e_prev) * A, the sum e_prev + ..., and the remodulating product e * d on the way out. Each rounding is at most
u = 2^-24 relative to a quantity no larger than the largest sample (in the demodulated domain everything is the sample over d,
and the comparison multiplies by d again), and an error made in an earlier update enters the next one times 1 - A <= 1. So after
K updates the deviation from exact arithmetic is below
    6 * K * 2^-24 * max |sample|
(a short induction gives about ((K + 1) / 2 + 5) u max|sample|: the stated bound is some ten times looser than the worst case and
still four orders of magnitude below what a wrong weight does, see the two wrong references below). The float64 reference's own
error, 40 additions at 2^-53, is nothing beside it. The moments plane M blends with the same four blend roundings (subtraction,
weight, product, sum) a sample that is itself rounded: l = l(c / d) is one divide, three products and two sums, six roundings, so
    m1: (4 + 6) * K * 2^-24 * max |l|;      m2: l * l doubles l's relative error and rounds once, (4 + 13) * K * 2^-24 * max l^2.
The steered fold makes the same update per extra sample; its K is the number of frames before it plus the largest count.

THE BOUND HAS TEETH: the same checks against two deliberately wrong float64 references — a blend weight of 1 / (n + 2), and a
sparse non-owner that blends its block's sample too — must fail, and that is asserted; the first is applied to every form, the
sparse one included, at every size. (At 1 x 1 a sparse frame has no non-owner: there the second wrong reference is the right one,
which is asserted instead, and the wrong weight is what the sparse check is shown to reject.)"""
import numpy as np
import pytest

from test_sparse_host import np_owners
from test_temporal_host import make_camera
from test_temporal_motion_host import table

F = np.float32
D = np.float64
U = 2.0 ** -24
K = 40
SIZES = [(1, 1), (7, 5), (67, 35)]
BLOCKS = [2, 3, 4]
R_BLEND, R_M1, R_M2 = 6, 4 + 6, 4 + 13  # roundings per update, see the module docstring
LUMA = np.array([F(0.2126), F(0.7152), F(0.0722)], D)  # the header's binary32 constants, exactly


def rest_inputs(pkg, W, H):
    """One camera and its guides — every pixel a valid hit of node 0 on the plane z = -5 with the normal +z, albedo in [0.2, 1] — and
    K frames of float32 samples in [0, 4] from a fixed seed."""
    rng = np.random.default_rng(40 * 1000003 + 1009 * W + H)
    y, x = np.mgrid[0:H, 0:W].astype(F)
    hits = np.zeros(W * H, pkg.hit_dtype())
    P = np.stack([x * F(0.1) - F(0.05 * W), y * F(0.1) - F(0.05 * H), np.full((H, W), F(-5.0))], -1).reshape(-1, 3)
    hits["p"], hits["N"], hits["flags"], hits["node"] = P, (0.0, 0.0, 1.0), 1, 0
    hits["t"] = np.sqrt((P.astype(D) ** 2).sum(-1)).astype(F)
    albedo = np.zeros((W * H, 4), F)
    albedo[:, :3] = F(0.2) + F(0.8) * rng.random((W * H, 3), dtype=F)
    frames = np.empty((K, H, W, 4), F)
    frames[..., :3] = F(4.0) * rng.random((K, H, W, 3), dtype=F)
    frames[..., 3] = hits["t"].reshape(H, W)
    assert albedo[:, :3].min() >= F(0.2) and albedo[:, :3].max() <= 1 and frames[..., :3].max() <= 4
    return {"W": W, "H": H, "cam": make_camera(pkg, W, H), "hits": hits, "albedo": albedo, "frames": frames, "still": table("static", 1),
            "d": albedo[:, :3].reshape(H, W, 3).astype(D), "extra": F(4.0) * rng.random((15 * W * H, 4), dtype=F),
            "counts": rng.integers(0, 16, (H, W)).astype(np.uint32)}


def lum(e):
    return e @ LUMA


def running(x, cap=None, precap=None, off=0):
    """The float64 reference over the leading axis of x: e <- e + (x - e) / (n + off) with n = min(min(n_prev, precap) + 1, cap);
    -> (e per frame, n per frame). Without caps and with off == 0 it is the arithmetic mean, and is computed as one: sum / count.
    off == 1 is the wrong weight 1 / (n + 2) on a history of n."""
    J = len(x)
    if cap is None and precap is None and off == 0:
        count = np.arange(1, J + 1, dtype=D)
        return np.cumsum(x, axis=0) / count.reshape((J,) + (1,) * (x.ndim - 1)), count
    e, n, es, ns = np.zeros_like(x[0]), 0.0, [], []
    for j in range(J):
        n = (n if precap is None else min(n, precap)) + 1
        n = n if cap is None else min(n, cap)
        e = e + (x[j] - e) / (n + off)
        es.append(e)
        ns.append(n)
    return np.stack(es), np.array(ns, D)


def dense_ratios(inp, outs, x=None, cap=None, precap=None, off=0, kk=K, last_only=False):
    """outs: per frame (image [..., 4], history [3 or 4, ..., 4]) of a chain fed x [frames, ..., 3] (default: the K frames), or with
    last_only its last frame alone. -> the largest |deviation| / tolerance per quantity over the frames and pixels, and whether n
    was exact everywhere. kk: the number of updates the tolerance is taken for."""
    x = inp["frames"][..., :3].astype(D) if x is None else x
    d = inp["d"]
    cut = (lambda a: a[-1:]) if last_only else (lambda a: a)
    want, n = running(x, cap, precap, off)
    tol = R_BLEND * kk * U * float(np.abs(x).max())
    E = np.stack([h[0] for _, h in outs]).astype(D)
    res = {"E": float(np.abs(E[..., :3] * d - cut(want)).max() / tol),
           "image": float(np.abs(np.stack([o for o, _ in outs]).astype(D)[..., :3] - cut(want)).max() / tol),
           "n": bool((E[..., 3] == cut(n).reshape((-1,) + (1,) * (E.ndim - 2))).all())}
    if outs[0][1].shape[0] == 4:
        l = lum(x / d)
        M = np.stack([h[3] for _, h in outs]).astype(D)
        res["m1"] = float(np.abs(M[..., 0] - cut(running(l, cap, precap, off)[0])).max() / (R_M1 * kk * U * float(np.abs(l).max())))
        res["m2"] = float(np.abs(M[..., 1] - cut(running(l * l, cap, precap, off)[0])).max() / (R_M2 * kk * U * float((l * l).max())))
        assert not M[..., 2:].any()
    return res


def within(res):
    return res["n"] and all(v <= 1.0 for k, v in res.items() if k != "n")


def report(what, inp, res):
    print("%-28s %2dx%-2d deviation / tolerance: %s" % (what, inp["W"], inp["H"], ", ".join("%s %.4f" % (k, v) for k, v in res.items() if not isinstance(v, bool))))


def dense_chain(inp, form):
    """form(k, rgbz, hist_prev or None) -> (image, history): the K frames through it, each against the history of the one before."""
    outs, hist = [], None
    for k in range(K):
        out, hist = form(k, inp["frames"][k], hist)
        outs.append((out, hist))
    return outs


def host_forms(pkg, inp, desc):
    cam, hits, albedo, still = inp["cam"], inp["hits"], inp["albedo"], inp["still"]
    return {"plain": lambda k, f, h: pkg.temporal_accumulate(cam if k else None, cam, f, hits, albedo, h, desc),
            "motion": lambda k, f, h: pkg.temporal_accumulate_motion(cam if k else None, cam, f, hits, albedo, still, h, desc, 0),
            "moments": lambda k, f, h: pkg.temporal_accumulate_moments(cam if k else None, cam, f, hits, albedo, still, h, desc, 0)}


# ---- 1. plain, motion and moments forms -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("max_history", [K, 65535, 4])
def test_a_history_at_rest_is_the_mean_of_its_samples(pkg, size, max_history):
    inp = rest_inputs(pkg, *size)
    cap = None if max_history >= K else max_history  # at or above K the clamp is never reached: the arithmetic mean, n == j + 1
    for name, form in host_forms(pkg, inp, pkg.temporal_desc(*size, max_history=max_history)).items():
        outs = dense_chain(inp, form)
        res = dense_ratios(inp, outs, cap=cap)
        report("%s, max_history %d" % (name, max_history), inp, res)
        assert within(res), "%s form: %s" % (name, res)
        wrong = dense_ratios(inp, outs, cap=cap, off=1)
        assert wrong["E"] > 1 and wrong["image"] > 1 and wrong.get("m1", 2) > 1 and wrong.get("m2", 2) > 1, \
            "%s form: a reference with the weight 1 / (n + 2) passed the same check: %s" % (name, wrong)


# ---- 2. the gradient form with a constant lambda plane ------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_a_constant_lambda_caps_the_history_before_each_blend(pkg, size):
    W, H = size
    inp = rest_inputs(pkg, W, H)
    cam, hits, albedo, still = inp["cam"], inp["hits"], inp["albedo"], inp["still"]
    desc = pkg.temporal_desc(W, H, max_history=K)
    for L, precap in ((0.25, 3), (1.0, 0), (2.0, 0)):  # 1 / 0.25 - 1 = 3 exactly; lambda >= 1: the sample itself, n = 1
        lam = np.full(((H + 2) // 3, (W + 2) // 3), L, F)
        outs = dense_chain(inp, lambda k, f, h: pkg.temporal_accumulate_gradient(cam if k else None, cam, f, hits, albedo, still, h, desc, 0, lam))
        res = dense_ratios(inp, outs, precap=precap)
        report("gradient, lambda %g" % L, inp, res)
        assert within(res), "lambda %g: %s" % (L, res)
        if precap == 0:
            assert all(np.array_equal(o[..., :3], inp["frames"][k][..., :3] / albedo[:, :3].reshape(H, W, 3) * albedo[:, :3].reshape(H, W, 3))
                       for k, (o, _) in enumerate(outs)), "lambda >= 1 is the sample itself"
        else:
            wrong = dense_ratios(inp, outs, precap=precap, off=1)
            assert wrong["E"] > 1 and wrong["m1"] > 1 and wrong["m2"] > 1, "the weight 1 / (n + 2) passed the same check: %s" % wrong


# ---- 3. the sparse form -----------------------------------------------------------------------------------------------------------------
def owner_mask(W, H, B, k):
    x, y, _, _ = np_owners(W, H, B, k)
    own = np.zeros((H, W), bool)
    own[y, x] = True
    return own, (x + W * y).astype(np.uint32)


def sparse_chain(inp, B, form):
    """form(k, rgbt [SW * SH, 4], owner, hist_prev or None) -> (image, history, hole): block b's sample of frame k is the frame's pixel
    at its owner of rtu_sparse_rays' rule (np_owners)."""
    outs, hist = [], None
    for k in range(K):
        owner = owner_mask(inp["W"], inp["H"], B, k)[1]
        out, hist, hole = form(k, np.ascontiguousarray(inp["frames"][k].reshape(-1, 4)[owner]), owner, hist)
        outs.append((out, hist, hole))
    return outs


def sparse_ratios(inp, B, outs, non_owners_blend=False, off=0):
    """A pixel's E is the mean of the samples of exactly the frames in which it was the owner, n their count, M the means of l and
    l^2 of those; hole is 1 exactly where a pixel has been the owner in no frame so far. non_owners_blend: the wrong reference in
    which every pixel of a block takes the block's sample; off == 1: the wrong weight 1 / (n + 2), which gives sum / (count + 1)."""
    W, H, d = inp["W"], inp["H"], inp["d"]
    x = inp["frames"][..., :3].astype(D)
    tol = R_BLEND * K * U * float(np.abs(x).max())
    lmax = float(np.abs(lum(x / d)).max())
    s, s1, s2, cnt = np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    yg, xg = np.mgrid[0:H, 0:W]
    sw = (W + B - 1) // B
    res = {"E": 0.0, "image": 0.0, "m1": 0.0, "m2": 0.0, "n": True, "hole": True, "carried": True}
    for k, (out, hist, hole) in enumerate(outs):
        own, owner = owner_mask(W, H, B, k)
        assert own.sum() == len(owner) == sw * ((H + B - 1) // B), "one owner per block"
        c = x[k]
        if non_owners_blend:
            c = x[k].reshape(-1, 3)[owner][(xg // B) + sw * (yg // B)] * d / d.reshape(-1, 3)[owner][(xg // B) + sw * (yg // B)]
            own = np.ones((H, W), bool)
        l = lum(c / d)
        s, s1, s2, cnt = s + own[..., None] * c, s1 + own * l, s2 + own * l * l, cnt + own
        has = cnt > 0
        E, M = hist[0].astype(D), hist[3].astype(D)
        div = np.maximum(cnt, 1) + off
        res["E"] = max(res["E"], float(np.abs((E[..., :3] * d - s / div[..., None])[has]).max() / tol))
        res["image"] = max(res["image"], float(np.abs((out[..., :3].astype(D) - s / div[..., None])[has]).max() / tol))
        res["m1"] = max(res["m1"], float(np.abs((M[..., 0] - s1 / div)[has]).max() / (R_M1 * K * U * lmax)))
        res["m2"] = max(res["m2"], float(np.abs((M[..., 1] - s2 / div)[has]).max() / (R_M2 * K * U * lmax * lmax)))
        res["n"] &= bool((E[..., 3] == cnt).all())
        res["hole"] &= bool(np.array_equal(hole == 1, ~has) and ((hole == 0) | (hole == 1)).all())
        if not non_owners_blend:
            prev = outs[k - 1][1] if k else np.zeros_like(hist)
            planes = (0, 1, 2, 3) if k else (0, 3)  # (frame 0 has no previous P and N: they are the guides')
            res["carried"] &= all(np.array_equal(hist[p].view(np.uint32)[~own], prev[p].view(np.uint32)[~own]) for p in planes)
    return res


def sparse_within(res):
    return res["n"] and res["hole"] and res["carried"] and all(res[k] <= 1.0 for k in ("E", "image", "m1", "m2"))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("B", BLOCKS)
def test_a_sparse_history_is_the_mean_of_the_frames_a_pixel_owned(pkg, size, B):
    W, H = size
    inp = rest_inputs(pkg, W, H)
    cam, hits, albedo, still = inp["cam"], inp["hits"], inp["albedo"], inp["still"]
    desc, sd = pkg.temporal_desc(W, H, max_history=K), pkg.sparse_desc(block=B)
    outs = sparse_chain(inp, B, lambda k, rgbt, owner, h: pkg.temporal_accumulate_sparse(cam if k else None, cam, rgbt, owner, hits, albedo, still, h, desc, sd, 0))
    res = sparse_ratios(inp, B, outs)
    report("sparse, block %d" % B, inp, res)
    assert sparse_within(res), res
    wrong = sparse_ratios(inp, B, outs, off=1)
    assert wrong["E"] > 1 and wrong["image"] > 1 and wrong["m1"] > 1 and wrong["m2"] > 1, "the weight 1 / (n + 2) passed the same check: %s" % wrong
    wrong = sparse_ratios(inp, B, outs, non_owners_blend=True)
    if size == (1, 1):
        assert sparse_within(dict(wrong, carried=True)), "one pixel: it owns every frame, and the wrong reference is the right one"
    else:
        assert wrong["E"] > 1 and wrong["image"] > 1 and wrong["m1"] > 1 and wrong["m2"] > 1 and not wrong["n"] and not wrong["hole"], \
            "a reference whose non-owners blend passed the same check: %s" % wrong


# ---- 4. the steered fold ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("max_history", [K, 4])
def test_the_fold_is_the_mean_over_history_and_extra_samples(pkg, size, max_history):
    """rtu_temporal_refine after n = 5 frames at rest: a pixel with c extra samples holds the mean over its 5 + c samples (the
    recursion clamped at max_history, where that is reached) and n = min(5 + c, max_history); a pixel with none passes bit for bit."""
    W, H = size
    n0 = 5
    inp = rest_inputs(pkg, W, H)
    cam, hits, albedo, still = inp["cam"], inp["hits"], inp["albedo"], inp["still"]
    desc = pkg.temporal_desc(W, H, max_history=max_history)
    out = hist = None
    for k in range(n0):
        out, hist = pkg.temporal_accumulate_moments(cam if k else None, cam, inp["frames"][k], hits, albedo, still, hist, desc, 0)
    counts = inp["counts"]
    offsets = (np.cumsum(counts.reshape(-1)) - counts.reshape(-1)).astype(np.uint32).reshape(H, W)
    rgbt = inp["extra"][:int(counts.sum())]
    got, folded = pkg.temporal_refine(hist, out, hits, albedo, counts, offsets, rgbt, desc)
    none = counts == 0
    assert np.array_equal(folded.view(np.uint32)[:, none], hist.view(np.uint32)[:, none]) and np.array_equal(got.view(np.uint32)[none], out.view(np.uint32)[none])
    assert np.array_equal(folded[1:3].view(np.uint32), hist[1:3].view(np.uint32)) and np.array_equal(got[..., 3].view(np.uint32), out[..., 3].view(np.uint32))
    worst, wrong = {"n": True}, {"n": True}
    cap = None if max_history >= n0 + 15 else max_history
    for c in range(1, 16):  # the pixels with c extra samples, as one chain of 5 + c frames each
        sel = np.argwhere(counts == c)
        if not len(sel):
            continue
        ys, xs = sel[:, 0], sel[:, 1]
        extra = np.stack([rgbt[offsets[ys, xs] + j][:, :3] for j in range(c)])      # [c, pixels, 3]
        x = np.concatenate([inp["frames"][:n0, ys, xs, :3], extra]).astype(D)       # [5 + c, pixels, 3]
        last = [(got[ys, xs], folded[:, ys, xs])]
        for acc, off in ((worst, 0), (wrong, 1)):
            res = dense_ratios({"d": inp["d"][ys, xs]}, last, x=x, cap=cap, off=off, kk=n0 + 15, last_only=True)
            for key, v in res.items():
                acc[key] = (acc["n"] and v) if key == "n" else max(acc.get(key, 0.0), v)
    report("fold, max_history %d" % max_history, inp, worst)
    assert within(worst), worst
    assert wrong["E"] > 1 and wrong["image"] > 1 and wrong["m1"] > 1 and wrong["m2"] > 1, "the weight 1 / (n + 2) passed the same check: %s" % wrong
