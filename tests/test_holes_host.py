"""The host forms of hole rays (rtu_hole_allocation, rtu_hole_fold; include/rtu_render.h "Hole rays") — the executable statements of the
rules, which the device forms must reproduce bit for bit (tests/test_gpu_holes.py) — against an integer numpy restatement, against
rtu_camera_sample_rays and the moments form, along a chain of sparse frames, and their effect on the oracle's own path-traced
samples. No GPU.

The hole planes are those rtu_temporal_accumulate_sparse writes on the chains of tests/test_sparse_host.py."""
import ctypes

import numpy as np
import pytest

from test_denoise_host import SIZES, bits, oracle_guides
from test_sparse_host import BLOCKS, QUALITY_FRAMES, owners_of, rmse
from test_steer_host import lens_camera, mix32
from test_temporal_host import chain_cameras, chain_inputs, orbit_scene
from test_temporal_motion_host import table

F = np.float32
U = np.uint32
RTU_RAY_HIT = 1
BUDGET_MAX = 1 << 26


def valid_of(hits, H, W):
    return ((hits["flags"] & RTU_RAY_HIT) != 0).reshape(H, W)


def finite_samples(rgbz):
    """The image with every sample that has a channel that is not finite replaced by a grey one."""
    out = rgbz.copy()
    bad = ~np.isfinite(out[..., :3]).all(-1)
    out[bad, :3] = 0.5
    return out


def sparse_frames(pkg, W, H, B, n_frames, seed=777, clean=False):
    """n_frames frames of a sparse chain on a moving camera (the cameras of chain X of test_temporal_host, walked round and round; the
    inputs of chain_inputs under consecutive seeds): per frame (camera, previous camera, owner, rgbt, hits, albedo, rgbz). clean: no
    sample has a channel that is not finite."""
    cams = chain_cameras(pkg, W, H)["X"]
    inputs = []
    while len(inputs) < n_frames:
        inputs += chain_inputs(pkg, W, H, seed + len(inputs))
    frames = []
    for k in range(n_frames):
        rgbz, hits, albedo = inputs[k]
        if clean:
            rgbz = finite_samples(rgbz)
        owner = owners_of(W, H, B, k)
        frames.append((cams[k % len(cams)], cams[(k - 1) % len(cams)] if k else None, owner, rgbz.reshape(-1, 4)[owner].copy(), hits, albedo, rgbz))
    return frames


def hole_planes(pkg, W, H, B, n_frames=3):
    """(hole plane, hits, history, image, albedo) of the first frames of a sparse chain, the history carried from frame to frame."""
    desc, sd, motion = pkg.temporal_desc(W, H), pkg.sparse_desc(block=B), table("static")
    hist, res = None, []
    for cam, prev, owner, rgbt, hits, albedo, _ in sparse_frames(pkg, W, H, B, n_frames):
        out, hist, hole = pkg.temporal_accumulate_sparse(prev, cam, rgbt, owner, hits, albedo, motion, hist, desc, sd)
        res.append((hole, hits, hist, out, albedo))
    return res


# ---- 1. the allocation ----------------------------------------------------------------------------------------------------------------
def np_hole_allocation(hole, hits, budget, k):
    """Rule 1 restated in integer arithmetic: (counts, offsets, total, the weights, whether the scan cut)."""
    H, W = hole.shape
    w = ((hole == 1) & valid_of(hits, H, W)).reshape(-1).astype(np.uint64)
    wsum = int(w.sum())
    if wsum == 0:
        z = np.zeros((H, W), U)
        return z, z.copy(), 0, w, False
    pix = np.arange(H * W, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = (mix32(pix.astype(U) + U(0x9e3779b9) * U((k + 1) & 0xffffffff)) >> U(16)).astype(np.uint64)
    c = np.minimum((np.uint64(budget) * w + ((h * np.uint64(wsum)) >> np.uint64(16))) // np.uint64(wsum), np.uint64(1))
    o = np.cumsum(c) - c
    offs = np.minimum(o, np.uint64(budget))
    cnt = np.minimum(c, np.uint64(budget) - offs)
    return cnt.astype(U).reshape(H, W), offs.astype(U).reshape(H, W), min(int(c.sum()), budget), w, int(c.sum()) > budget


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_allocation_equals_the_integer_restatement(pkg, size, B):
    W, H = size
    seen = dict(cut=0, uncut=0, holes=0, invalid_holes=0, taken=0)
    for hole, hits, _, _, _ in hole_planes(pkg, W, H, B):
        valid = valid_of(hits, H, W)
        candidate = (hole == 1) & valid
        wsum = int(candidate.sum())
        seen["holes"] += wsum
        seen["invalid_holes"] += int(((hole == 1) & ~valid).sum())
        for budget in sorted({0, 1, max(wsum - 1, 0), wsum, BUDGET_MAX}):
            for k in (0, 1, 0xffffffff):
                counts, offsets, total = pkg.hole_allocation(hole, hits, pkg.hole_desc(budget=budget, frame_index=k))
                wc, wo, wt, w, cut = np_hole_allocation(hole, hits, budget, k)
                assert np.array_equal(counts, wc) and np.array_equal(offsets, wo) and total == wt, (budget, k)
                assert counts.max() <= 1 and not counts[~candidate].any(), "a ray for a pixel that is no VALID hole"
                flat = counts.reshape(-1)
                assert np.array_equal(offsets.reshape(-1), np.minimum(np.cumsum(flat, dtype=np.uint64) - flat, budget).astype(U)), \
                    "offsets is not the exclusive scan of counts"
                assert total == int(flat.sum(dtype=np.uint64)) and total <= budget
                assert (total == wsum) == (budget >= wsum), "total = Wsum exactly when budget >= Wsum"
                if budget >= wsum:
                    assert np.array_equal(counts == 1, candidate), "with the full budget every VALID hole gets its ray"
                seen["cut" if cut else "uncut"] += 1
                seen["taken"] += total
        if wsum >= 2:  # (Wsum / 2 is no ray at all for a single hole)
            visits = np.zeros((H, W), np.int64)
            for k in range(64):
                counts, _, total = pkg.hole_allocation(hole, hits, pkg.hole_desc(budget=wsum // 2, frame_index=k))
                assert total <= wsum // 2
                visits += counts
                cut = np_hole_allocation(hole, hits, wsum // 2, k)[4]
                seen["cut" if cut else "uncut"] += 1
            assert (visits[candidate] >= 1).all(), "over 64 frames at half the budget %d of %d holes never got a ray" % (int((visits[candidate] == 0).sum()), wsum)
            assert not visits[~candidate].any()
    print("%dx%d B %d: %s" % (W, H, B, seen))
    if B == 1 or size == (1, 1):
        assert seen["holes"] == 0 and seen["taken"] == 0, "every pixel is an owner: no hole, no ray"
    else:
        assert seen["holes"] and seen["taken"] and seen["cut"] and seen["uncut"], "a frame cut by the scan and an uncut one must occur: %s" % seen
    if B > 1 and size == (67, 35):
        assert seen["invalid_holes"], "an invalid hole, which takes no ray"


def test_allocation_defaults_and_refusals(pkg):
    W, H, B = 7, 5, 2
    hole, hits, _, _, _ = hole_planes(pkg, W, H, B, 1)[0]
    counts, offsets, total = np.zeros((H, W), U), np.zeros((H, W), U), ctypes.c_uint32(0)
    d = pkg.hole_desc(W, H)
    assert ctypes.sizeof(d) == 32 and d.budget == 0 and d.frame_index == 0 and not any(d.reserved)
    raw = pkg.RtuHoleDesc()
    assert pkg.hip.rtu_hole_defaults(ctypes.byref(raw)) == pkg.RTU_OK and raw.width == 0 and raw.height == 0 and raw.budget == 0
    assert pkg.hip.rtu_hole_defaults(None) == pkg.RTU_ERR_ARG

    def call(d=d, hole=hole, hits=hits, counts=counts, offsets=offsets, total=total):
        p = lambda a: a.ctypes.data if a is not None else None
        return pkg.hip.rtu_hole_allocation(ctypes.byref(d) if d is not None else None, p(hole), p(hits), p(counts), p(offsets),
                                           ctypes.byref(total) if total is not None else None)
    assert call() == pkg.RTU_OK and total.value == 0 and not counts.any()
    assert call(d=pkg.hole_desc(W, H, budget=BUDGET_MAX)) == pkg.RTU_OK and total.value > 0
    assert call(d=pkg.hole_desc(W, H, budget=BUDGET_MAX + 1)) == pkg.RTU_ERR_ARG
    for size in ((0, 0), (0, H), (W, 0), (-1, H), (65537, 1), (65536, 65536)):
        assert call(d=pkg.hole_desc(*size)) == pkg.RTU_ERR_ARG, size
    for i in range(4):
        bad = pkg.hole_desc(W, H)
        bad.reserved[i] = 1
        assert call(d=bad) == pkg.RTU_ERR_ARG
    for name in ("d", "hole", "hits", "counts", "offsets", "total"):
        assert call(**{name: None}) == pkg.RTU_ERR_ARG, name
    marks = np.full((H, W), 2, np.uint8)  # marks other than 1 are no holes
    assert call(d=pkg.hole_desc(W, H, budget=BUDGET_MAX), hole=marks) == pkg.RTU_OK and total.value == 0


# ---- 2. the rays: rtu_extra_sample_rays with max_extra = 1 ------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BLOCKS[1:])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_hole_rays_are_camera_sample_rays_of_the_second_half(pkg, size, B):
    W, H = size
    hole, hits, _, _, _ = hole_planes(pkg, W, H, B, 1)[0]
    seen = 0
    for S in (1, 3, 4096):
        frame, big = lens_camera(pkg, W, H, S), lens_camera(pkg, W, H, 2 * S)
        assert frame.dof > 0
        for k, budget in ((0, BUDGET_MAX), (1, BUDGET_MAX), (S + 2, max(int((hole == 1).sum()) // 2, 1)), (0xffffffff, BUDGET_MAX)):
            counts, offsets, total = pkg.hole_allocation(hole, hits, pkg.hole_desc(budget=budget, frame_index=k))
            rays, keys, owner = pkg.extra_sample_rays(frame, counts, offsets, pkg.steer_desc(budget=budget, max_extra=1, frame_index=k))
            assert len(rays) == total and np.array_equal(owner, np.flatnonzero(counts.reshape(-1)).astype(U))
            assert np.array_equal(offsets.reshape(-1)[owner], np.arange(total, dtype=U)), "owner[offsets_p] = p"
            sample = S + k % S
            assert S <= sample < 2 * S, "disjoint from the samples 0 .. S - 1 the owners walk through"
            want_rays, want_keys = pkg.camera_sample_rays(big, sample)
            assert rays.tobytes() == want_rays[owner].tobytes() and np.array_equal(keys, want_keys[owner]), (S, k)
            seen += total
    assert size == (1, 1) or seen > 0


def test_hole_rays_need_two_s_samples(pkg):
    W, H = 7, 5
    hole, hits, _, _, _ = hole_planes(pkg, W, H, 2, 1)[0]
    counts, offsets, total = pkg.hole_allocation(hole, hits, pkg.hole_desc(budget=BUDGET_MAX))
    assert total > 0
    sd = pkg.steer_desc(budget=BUDGET_MAX, max_extra=1)
    assert len(pkg.extra_sample_rays(lens_camera(pkg, W, H, 32768), counts, offsets, sd)[0]) == total  # 2 S == 65536
    with pytest.raises(pkg.RtuError):
        pkg.extra_sample_rays(lens_camera(pkg, W, H, 32769), counts, offsets, sd)


# ---- 3. the fold ------------------------------------------------------------------------------------------------------------------------
ODD = (F(np.nan), F(np.inf), F(3e38), -F(np.inf), F(-0.25), F(-3e38))


def fold_samples(total, seed):
    """`total` samples {r, g, b, t}: positive noise, every third with one channel NaN, infinite, so large that the square of the
    luminance overflows, or negative."""
    rng = np.random.default_rng(seed)
    rgbt = rng.uniform(0.01, 2.0, (total, 4)).astype(F)
    for j, i in enumerate(range(0, total, 3)):
        rgbt[i, j % 3] = ODD[j % len(ODD)]
    return rgbt


def check_fold(pkg, cam, hist, out, hole, hits, albedo, counts, offsets, rgbt, seen):
    """rtu_hole_fold against rtu_temporal_accumulate_moments without a previous history on an image that holds each pixel's sample."""
    H, W = hole.shape
    got_out, got_hist, got_hole = pkg.hole_fold(hist, out, hole, hits, albedo, counts, offsets, rgbt)
    valid = valid_of(hits, H, W)
    selected = (counts.reshape(H, W) >= 1) & (hole == 1) & valid
    dense = np.full((H, W, 4), 0.25, F)
    dense[counts.reshape(H, W) >= 1] = rgbt[offsets.reshape(-1)[counts.reshape(-1) >= 1]]
    fresh_out, fresh_hist = pkg.temporal_accumulate_moments(None, cam, dense, hits, albedo, table("static"), None, pkg.temporal_desc(W, H))
    finite = np.isfinite(dense[..., :3]).all(-1)
    folded = selected & finite
    want_hist, want_out, want_hole = hist.copy(), out.copy(), hole.copy()
    want_hist[0][folded] = fresh_hist[0][folded]
    want_hist[3][folded] = fresh_hist[3][folded]
    want_out[folded, :3] = fresh_out[folded, :3]
    want_hole[folded] = 0
    assert (fresh_hist[0][folded][:, 3] == 1).all(), "the moments form gave a folded pixel n == 1"
    assert np.array_equal(bits(got_hist), bits(want_hist)), "E, M of a folded pixel are not the moments form's, or another word changed"
    assert np.array_equal(bits(got_out), bits(want_out)), "rgb of a folded pixel is not the moments form's, or z or another pixel changed"
    assert np.array_equal(got_hole, want_hole), "the hole plane: 0 at the folded pixels, every other byte unchanged"
    assert (got_hole[selected & ~finite] == 1).all(), "a sample that is not finite leaves the pixel a hole"
    skipped_moments = folded & (got_hist[3][..., 0] == 0) & (got_hist[3][..., 1] == 0) & (got_hist[0][..., :3] != 0).any(-1)
    seen["folded"] += int(folded.sum())
    seen["not_finite"] += int((selected & ~finite).sum())
    seen["moments_skipped"] += int(skipped_moments.sum())
    seen["not_selected"] += int(((hole == 1) & valid & (counts.reshape(H, W) == 0)).sum())
    seen["count_on_no_hole"] += int(((counts.reshape(H, W) >= 1) & ~selected).sum())
    seen["negative"] += int((folded & (dense[..., :3] < 0).any(-1)).sum())
    return got_out, got_hist, got_hole


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_fold_equals_the_moments_form_of_a_fresh_pixel(pkg, size, B):
    W, H = size
    seen = dict(folded=0, not_finite=0, moments_skipped=0, not_selected=0, count_on_no_hole=0, negative=0)
    cams = chain_cameras(pkg, W, H)["X"]
    for k, (hole, hits, hist, out, albedo) in enumerate(hole_planes(pkg, W, H, B)):
        wsum = int(((hole == 1) & valid_of(hits, H, W)).sum())
        for budget in (BUDGET_MAX, (2 * wsum) // 3):
            counts, offsets, total = pkg.hole_allocation(hole, hits, pkg.hole_desc(budget=budget, frame_index=k))
            # two counts the allocation would not give — a pixel that is no hole, an invalid hole — name a sample of their own
            counts, offsets = counts.copy(), offsets.copy()
            extra = [i for i in (np.flatnonzero(hole.reshape(-1) == 0)[:1], np.flatnonzero((hole.reshape(-1) == 1) & ~valid_of(hits, H, W).reshape(-1))[:1])
                     if len(i)]
            for j, i in enumerate(extra):
                counts.reshape(-1)[i], offsets.reshape(-1)[i] = 1, total + j
            rgbt = fold_samples(total + len(extra), 31 * k + B)
            check_fold(pkg, cams[k % len(cams)], hist, out, hole, hits, albedo, counts, offsets, rgbt, seen)
    print("%dx%d B %d: %s" % (W, H, B, seen))
    if B > 1 and size == (67, 35):
        assert all(seen.values()), "folded, skipped as not finite, moments skipped, not selected, a count on no hole, a negative sample: %s" % seen
    if B > 1 and size == (7, 5):
        assert seen["folded"] and seen["not_finite"] and seen["not_selected"], seen


def test_fold_refusals(pkg):
    W, H, B = 7, 5, 2
    hole, hits, hist, out, albedo = hole_planes(pkg, W, H, B, 1)[0]
    counts, offsets, total = pkg.hole_allocation(hole, hits, pkg.hole_desc(budget=BUDGET_MAX))
    assert total > 1
    rgbt = fold_samples(total, 5)
    d = pkg.hole_desc(W, H)
    keep = [a.copy() for a in (hist, out, hole)]

    def call(d=d, hist=hist, out=out, hole=hole, hits=hits, albedo=albedo, counts=counts, offsets=offsets, rgbt=rgbt, n=total):
        p = lambda a: a.ctypes.data if a is not None else None
        return pkg.hip.rtu_hole_fold(ctypes.byref(d) if d is not None else None, p(hist), p(out), p(hole), p(hits), p(albedo), p(counts), p(offsets),
                                     p(rgbt), n)
    for name in ("d", "hist", "out", "hole", "hits", "albedo", "counts", "offsets", "rgbt"):
        assert call(**{name: None}) == pkg.RTU_ERR_ARG, name
    assert call(d=pkg.hole_desc(W, H, budget=BUDGET_MAX + 1)) == pkg.RTU_ERR_ARG
    assert call(d=pkg.hole_desc(0, 0)) == pkg.RTU_ERR_ARG and call(d=pkg.hole_desc(65537, 1)) == pkg.RTU_ERR_ARG
    bad = pkg.hole_desc(W, H)
    bad.reserved[2] = 1
    assert call(d=bad) == pkg.RTU_ERR_ARG
    assert call(n=total - 1) == pkg.RTU_ERR_ARG, "a pixel whose offsets_p + counts_p exceeds n_rays"
    assert call(n=BUDGET_MAX + 1) == pkg.RTU_ERR_ARG
    two = counts.copy()
    two.reshape(-1)[np.flatnonzero(counts.reshape(-1))[0]] = 2
    assert call(counts=two, n=total + 1) == pkg.RTU_ERR_ARG, "a count above 1"
    far = offsets.copy()
    far.reshape(-1)[np.flatnonzero(counts.reshape(-1))[-1]] = total
    assert call(offsets=far) == pkg.RTU_ERR_ARG
    for a, b in zip((hist, out, hole), keep):
        assert np.array_equal(bits(a) if a.dtype == F else a, bits(b) if b.dtype == F else b), "a refused call wrote something"
    assert call(rgbt=None, n=0, counts=np.zeros_like(counts), offsets=np.zeros_like(offsets)) == pkg.RTU_OK  # no rays: nothing to read
    assert call() == pkg.RTU_OK and not np.array_equal(hole, keep[2])
    with pytest.raises(pkg.RtuError):
        pkg.hole_fold(keep[0], keep[1], keep[2], hits, albedo, two, offsets, rgbt)


# ---- 4. a chain ---------------------------------------------------------------------------------------------------------------------------
def run_chain(pkg, W, H, B, budget, with_holes=True):
    """2 B^2 + 1 frames of the sparse chain on a moving camera with finite samples; with_holes: allocation, fold (the hole samples are
    the frame's own image at those pixels) and fill, else the sparse session's steps alone. Per frame (image, history, hole plane
    before the fill, total)."""
    desc, sd, motion = pkg.temporal_desc(W, H), pkg.sparse_desc(block=B), table("static")
    hist, res = None, []
    for k, (cam, prev, owner, rgbt, hits, albedo, rgbz) in enumerate(sparse_frames(pkg, W, H, B, 2 * B * B + 1, seed=4242, clean=True)):
        out, hist, hole = pkg.temporal_accumulate_sparse(prev, cam, rgbt, owner, hits, albedo, motion, hist, desc, sd)
        total = 0
        if with_holes:
            counts, offsets, total = pkg.hole_allocation(hole, hits, pkg.hole_desc(budget=budget, frame_index=k))
            samples = rgbz.reshape(-1, 4)[np.flatnonzero(counts.reshape(-1))] * F(0.5)
            out, hist, hole = pkg.hole_fold(hist, out, hole, hits, albedo, counts, offsets, samples)
        out = pkg.sparse_fill(out, hole, hits, albedo, owner, rgbt, desc, sd)
        res.append((out, hist, hole, total, hits, owner))
    return res


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("size", SIZES[1:], ids=lambda s: "%dx%d" % s)
def test_a_chain_with_the_full_budget_leaves_no_valid_hole(pkg, size, B):
    W, H = size
    full = run_chain(pkg, W, H, B, BUDGET_MAX)
    assert len(full) == 2 * B * B + 1
    rays = []
    for k, (out, hist, hole, total, hits, owner) in enumerate(full):
        valid = valid_of(hits, H, W)
        assert not (hole == 1)[valid].any(), "frame %d: a VALID pixel is still a hole" % k
        assert (hist[0][..., 3][valid] >= 1).all(), "frame %d: a VALID pixel without history" % k
        rays.append(total)
        if k == 0:
            is_owner = np.zeros(W * H, bool)
            is_owner[owner] = True
            assert (hist[0][..., 3][valid] == 1).all(), "after frame 0, n == 1 on every VALID pixel"
            assert np.array_equal(hole == 1, ~valid & ~is_owner.reshape(H, W)), "after frame 0 the hole plane holds exactly the invalid non-owners"
            assert total == int((valid & ~is_owner.reshape(H, W)).sum())
    print("%dx%d B %d: hole rays per frame %s" % (W, H, B, rays))
    if B > 1:
        assert rays[0] > 0 and sum(rays[1:]) > 0, "hole rays in frame 0 and, on the moving camera, after it: %s" % rays


@pytest.mark.parametrize("B", BLOCKS)
def test_a_chain_with_budget_0_is_the_sparse_chain(pkg, B):
    W, H = 67, 35
    for a, b in zip(run_chain(pkg, W, H, B, 0), run_chain(pkg, W, H, B, 0, with_holes=False)):
        assert a[3] == 0
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])


# ---- 5. quality, on the oracle alone ------------------------------------------------------------------------------------------------------
S_ORACLE = 16
CUT_DEG = 20.0
TAG = "p11_p2_120x68"


class OracleChain:
    """A sparse chain (B = 2, recipe P, S = 16: the setup of DESIGN.md section 28) on the oracle's samples through the host forms, with
    hole rays of `budget`: frame k shades its owners in sample (k div 4) mod 16 and its holes in sample 16 + k mod 16 of the frame with
    32 samples."""

    def __init__(self, pkg, orc, golden, budget):
        self.pkg, self.orc, self.budget = pkg, orc, budget
        g = golden(TAG)
        self.scene, self.W, self.H = g.scene(pkg), g.width, g.height
        self.desc, self.vdesc, self.sd = pkg.temporal_desc(self.W, self.H), pkg.variance_desc(), pkg.sparse_desc(block=2)
        self.motion = table("static", self.scene.desc.n_nodes)
        self.distance = float(oracle_guides(pkg, orc, self.scene, self.W, self.H)[0][(self.H // 2) * self.W + self.W // 2]["t"])
        self.hist = self.prev = None
        self.k = 0

    def frame(self, angle_deg, cache):
        """One frame through the orbit camera at angle_deg: {raw, acc, filt: RMSE against 256 spp, holes, rays}. cache: what the two
        chains share per (angle, frame index) — scene, guides, sample images, reference."""
        pkg, orc, W, H, k = self.pkg, self.orc, self.W, self.H, self.k
        key = (angle_deg, k)
        if key not in cache:
            s = orbit_scene(pkg, self.scene, 1, self.distance, angle_deg)
            if ("ref", angle_deg) not in cache:
                cache[("ref", angle_deg)] = (oracle_guides(pkg, orc, s, W, H), orc.render_paths(s, W, H, 256, threads=8)[0])
            cache[key] = (s, orc.sample_images(s, W, H, S_ORACLE, (k // 4) % S_ORACLE, 1, gi=True, threads=8)[0],
                          orc.sample_images(s, W, H, 2 * S_ORACLE, S_ORACLE + k % S_ORACLE, 1, gi=True, threads=8)[0])
        s, sample, second = cache[key]
        (hits, albedo), ref = cache[("ref", angle_deg)]
        frame = pkg.frame_setup(s.desc.camera, W, H, samples=S_ORACLE, gather_bounces=4)
        owner = owners_of(W, H, 2, k)
        rgbt = np.asarray(sample, F).reshape(-1, 4)[owner]
        out, hist, hole = pkg.temporal_accumulate_sparse(self.prev, frame, rgbt, owner, hits, albedo, self.motion, self.hist, self.desc, self.sd)
        counts, offsets, total = pkg.hole_allocation(hole, hits, pkg.hole_desc(budget=self.budget, frame_index=k))
        picked = np.flatnonzero(counts.reshape(-1))
        out, hist, hole = pkg.hole_fold(hist, out, hole, hits, albedo, counts, offsets, np.asarray(second, F).reshape(-1, 4)[picked])
        out = pkg.sparse_fill(out, hole, hits, albedo, owner, rgbt, self.desc, self.sd)
        filtered = pkg.denoise_variance(out, hits, albedo, pkg.variance(hist, hits, self.vdesc), self.vdesc)
        self.hist, self.prev, self.k = hist, frame, k + 1
        raw = rmse(np.asarray(sample, F).reshape(H, W, 4), ref)
        return dict(raw=raw, acc=rmse(out, ref) / raw, filt=rmse(filtered, ref) / raw, holes=int(hole.sum()), rays=total)


def quality_rows(pkg, orc, golden):
    """{row: {budget: frame result}} for frame 0, the last of the 8 orbit frames and frames 0 .. 3 after the cut."""
    cache, rows = {}, {}
    for budget in (0, BUDGET_MAX):
        chain = OracleChain(pkg, orc, golden, budget)
        for k in range(QUALITY_FRAMES):
            r = chain.frame(0.25 * k, cache)
            if k == 0:
                rows.setdefault("frame 0", {})[budget] = r
        rows.setdefault("orbit, frame 7", {})[budget] = r
        for j in range(4):
            rows.setdefault("cut + %d" % j, {})[budget] = chain.frame(CUT_DEG, cache)
    return rows


# Measured RMSE ratios to the raw single sample's, p11_p2_120x68, recipe P, S = 16, B = 2, accumulated + filled /
# filtered; holes: what the fill had to fill, of 8160 pixels (at full budget those are the misses):
#                     budget 0                         full budget
#   frame 0           0.6371 / 0.2848  (6120 holes)    0.9904 / 0.1768  (6120 hole rays, 0 holes)
#   orbit, frame 7    0.5433 / 0.1730  (8)             0.4632 / 0.1530  (3 rays, 0)
#   cut + 0           0.4799 / 0.1855  (4092)          0.6109 / 0.1623  (3865 rays, 226)
#   cut + 1           0.5599 / 0.1737  (2775)          0.5874 / 0.1567
#   cut + 2           0.5829 / 0.1669  (1508)          0.5564 / 0.1567
#   cut + 3           0.6215 / 0.1622  (197)           0.5217 / 0.1562
# Each bound is the measured ratio plus 5 %. AFTER THE FILTER the full budget is better in every row, and that ordering is asserted.
# BEFORE THE FILTER it is WORSE at frame 0 and in the first two frames after the cut (0.9904 against 0.6371): a hole ray is one raw
# sample where the fill shows the mean of up to nine; that ordering is written down, not asserted, and no constant was tuned on it. On
# the orbit the full budget is better both ways, not indistinguishable: after 8 frames most pixels of the budget-0 chain have had two
# samples (their turn as owner came twice), those of the full-budget chain three.
QUALITY = {
    "frame 0": {0: (0.6690, 0.2991), BUDGET_MAX: (1.0400, 0.1857)},
    "orbit, frame 7": {0: (0.5705, 0.1817), BUDGET_MAX: (0.4864, 0.1607)},
    "cut + 0": {0: (0.5039, 0.1948), BUDGET_MAX: (0.6415, 0.1705)},
    "cut + 1": {0: (0.5879, 0.1824), BUDGET_MAX: (0.6168, 0.1646)},
    "cut + 2": {0: (0.6121, 0.1753), BUDGET_MAX: (0.5843, 0.1646)},
    "cut + 3": {0: (0.6526, 0.1704), BUDGET_MAX: (0.5478, 0.1641)},
}


def test_quality_on_the_oracle(pkg, orc, golden):
    rows = quality_rows(pkg, orc, golden)
    for name, row in rows.items():
        for budget, r in row.items():
            print("%s %s budget %s: raw RMSE %.5f; ratios: accumulated + filled %.4f, filtered %.4f; holes filled %d, hole rays %d"
                  % (TAG, name, "full" if budget else "0", r["raw"], r["acc"], r["filt"], r["holes"], r["rays"]))
    assert set(rows) == set(QUALITY)
    assert rows["frame 0"][BUDGET_MAX]["rays"] == rows["frame 0"][0]["holes"] > 0 and rows["cut + 0"][BUDGET_MAX]["rays"] > 0, "conditions on the input"
    for name, row in rows.items():
        for budget, r in row.items():
            acc, filt = QUALITY[name][budget]
            assert r["acc"] < acc and r["filt"] < filt, "%s, budget %d: RMSE ratios %.4f, %.4f" % (name, budget, r["acc"], r["filt"])
        assert row[BUDGET_MAX]["filt"] < row[0]["filt"], "%s: after the filter the full budget was better: %s" % (name, row)
