"""Ray sorting on the GPU (rtu_ray_order_device, rtu_permute_device, sort=True of the five ray entries; include/rtu_render.h "Ray
sorting"). The order is compared EXACTLY with np.argsort(ray_sort_keys(box, rays), kind="stable") — the host key function, itself
checked against a numpy restatement in tests/test_ray_sort_host.py — so kernel key, every digit pass, the scan across workgroups and
stability are all under one equality. The sorted forms of the entries are compared byte for byte with the unsorted answers to the same
shuffled batch, which the existing tests tie to the renders and the oracle."""
import ctypes

import numpy as np
import pytest

from test_mesh_update_host import clone
from test_ray_sort_host import BIG, F, INVALID, MISS, invalid_rays, make_rays, missed, unit

pytestmark = pytest.mark.gpu

TILE = 4096  # RTU_SORT_TILE: the pairs one workgroup of the sorter takes


class Dev:
    """A device buffer holding a copy of a numpy array (or `nbytes` bytes of 0xA5)."""

    def __init__(self, pkg, ctx, a=None, nbytes=0):
        self.pkg, self.ctx = pkg, ctx
        self.nbytes = int(a.nbytes if a is not None else nbytes)
        self.ptr = pkg.hip.rtu_device_alloc(ctx._h, max(self.nbytes, 16))
        assert self.ptr
        src = np.ascontiguousarray(a) if a is not None else np.full(self.nbytes, 0xA5, np.uint8)
        if self.nbytes:
            assert pkg.hip.rtu_copy_to_device(ctx._h, self.ptr, src.ctypes.data, self.nbytes) == 0

    def get(self, dtype=np.uint8):
        out = np.zeros(self.nbytes // np.dtype(dtype).itemsize, dtype)
        if self.nbytes:
            assert self.pkg.hip.rtu_copy_to_host(self.ctx._h, out.ctypes.data, self.ptr, self.nbytes) == 0  # waits for the device
        return out

    def free(self):
        self.pkg.hip.rtu_device_free(self.ctx._h, self.ptr)


def order_device(pkg, ctx, rays):
    """rtu_ray_order_device on a copy of `rays` in device memory, on the context's stream."""
    d_rays, d_order = Dev(pkg, ctx, rays), Dev(pkg, ctx, nbytes=4 * rays.size)
    try:
        ctx.ray_order_device(d_rays.ptr, rays.size, d_order.ptr, pkg.hip.rtu_context_stream(ctx._h))
        return d_order.get(np.uint32)
    finally:
        d_rays.free()
        d_order.free()


def expected(pkg, box, rays):
    keys = pkg.ray_sort_keys(box, rays)
    return keys, np.argsort(keys, kind="stable").astype(np.uint32)


@pytest.fixture(scope="module")
def p4(pkg, golden):
    return golden("p4_240x135").scene(pkg)


@pytest.fixture(scope="module")
def teapot(pkg, golden):
    return golden("teapot2_240x135").scene(pkg)


@pytest.fixture(scope="module")
def ctx(pkg, p4):
    """A context holding p4. Tests that upload something else use a context of their own."""
    c = pkg.Context(0)
    c.upload(p4)
    yield c
    c.close()


def mixed_rays(pkg, box, n, seed):
    """n rays around and inside `box`, every direction, some too short to reach it, and one invalid ray of each kind among them."""
    rng = np.random.RandomState(seed)
    mid, half = (box[:3] + box[3:]) * F(0.5), (box[3:] - box[:3]) * F(0.5)
    rays = make_rays(pkg, (mid + rng.standard_normal((n, 3)).astype(F) * half * F(0.8)).astype(F), unit(rng, n))
    rays["tmax"][::5] = half.min() * F(0.5)
    bad = invalid_rays(pkg)
    at = rng.permutation(n)[:min(n, len(bad))]
    rays[at] = bad[:len(at)]
    return rays


# 1 .. 65: one wavefront and a little more; TILE - 1, TILE, TILE + 1 (4097): one workgroup and the step to two; 70001: 18 workgroups,
# scan carries across them in every pass; 257 * TILE + 5: more tiles than the scan kernel has threads (each takes two)
@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 70001, 257 * TILE + 5])
def test_order_is_the_stable_argsort(pkg, ctx, n):
    box = ctx.ray_sort_box()
    rays = mixed_rays(pkg, box, n, n)
    keys, want = expected(pkg, box, rays)
    got = order_device(pkg, ctx, rays)
    print("n %d: %d distinct keys, %d miss, %d invalid" % (n, len(np.unique(keys)), int(missed(keys).sum()), int((keys == INVALID).sum())))
    assert np.array_equal(got, want)
    if n >= 65:
        assert len(np.unique(keys)) > n // 4 and (keys == INVALID).sum() == 7 and missed(keys).any()
    if n >= 70001:
        for shift in (0, 8, 16, 24):  # every digit pass has something to do
            assert len(np.unique((keys >> shift) & 0xFF)) > 3
    if n == 70001:
        assert np.array_equal(ctx.ray_order(rays), want)  # the host form


def crafted(pkg, box):
    """name -> rays whose keys have the stated structure (asserted on the host keys by the test)."""
    rng = np.random.RandomState(11)
    lo, ext = box[:3], box[3:] - box[:3]
    down = np.array([0, 0, -1], F)
    centre = lambda c: (lo + (np.asarray(c, F) + F(0.5)) / F(16) * ext).astype(F)  # the middle of cell c
    out = {}
    out["equal"] = make_rays(pkg, np.tile(centre([3, 9, 5]), (5000, 1)), down)
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
    out["distinct"] = make_rays(pkg, centre(g)[rng.permutation(4096)], down)  # every cell once
    sent = make_rays(pkg, np.tile(box[3:] + F(1), (6000, 1)), np.array([0, 0, 1], F))  # beside the box, pointing away: one key
    sent["tmax"][rng.permutation(6000)[:2500]] = -1  # invalid
    out["sentinels"] = sent
    top = g[(g % 4 == 0).all(1)]  # cells 0, 4, 8, 12 per axis: spatial bits 6 .. 11, key bits 24 .. 29
    rays = make_rays(pkg, centre(top)[rng.randint(0, len(top), 9000)], down)
    rays["org"][rng.permutation(9000)[:300]] = box[3:] + F(1)  # beside the box, the same direction: a miss — bit 30 and that direction
    out["top digit"] = rays
    # directions whose octahedral cells differ in their low 4 bits only, from one point: key bits 0 .. 7
    qu, qv = rng.randint(0, 16, 7000) + 256 + 32, rng.randint(0, 16, 7000) + 256 + 48
    px, py = (qu + 0.5) / 256.0 - 1.0, (qv + 0.5) / 256.0 - 1.0
    d = np.stack([px, py, 1.0 - np.abs(px) - np.abs(py)], 1)
    out["bottom digit"] = make_rays(pkg, np.tile(centre([8, 8, 8]), (7000, 1)), (d / np.sqrt((d * d).sum(1))[:, None]).astype(F))
    return out


@pytest.mark.parametrize("case", ["equal", "distinct", "sentinels", "top digit", "bottom digit"])
def test_order_of_crafted_keys(pkg, ctx, case):
    box = ctx.ray_sort_box()
    rays = crafted(pkg, box)[case]
    keys, want = expected(pkg, box, rays)
    if case == "equal":
        assert len(np.unique(keys)) == 1 and keys[0] < MISS and np.array_equal(want, np.arange(rays.size))  # stability: the identity
    elif case == "distinct":
        assert len(np.unique(keys)) == rays.size
    elif case == "sentinels":
        assert len(np.unique(keys)) == 2 and (keys == INVALID).sum() == 2500 and missed(keys).sum() == 3500
    elif case == "top digit":
        ordinary = keys[keys < MISS]
        assert len(np.unique(ordinary >> 24)) == 64 and len(np.unique(ordinary & 0xFFFFFF)) == 1
        assert missed(keys).sum() == 300 and len(np.unique(keys & 0xFFFFFF)) == 1 and len(np.unique(keys >> 24)) == 65
    else:
        assert len(np.unique(keys >> 8)) == 1 and len(np.unique(keys & 0xFF)) == 256
    assert np.array_equal(order_device(pkg, ctx, rays), want)


def test_order_is_a_function_of_rays_and_scene(pkg, ctx, p4):
    box = ctx.ray_sort_box()
    rays = mixed_rays(pkg, box, 3 * TILE + 77, 5)
    a = order_device(pkg, ctx, rays)
    b = order_device(pkg, ctx, rays)  # warm: the scratch is there
    fresh = pkg.Context(0)
    try:
        fresh.upload(p4)
        c = order_device(pkg, fresh, rays)
    finally:
        fresh.close()
    assert a.tobytes() == b.tobytes() == c.tobytes()
    assert np.array_equal(a, expected(pkg, box, rays)[1])


@pytest.mark.parametrize("elem", [1, 4, 16, 32, 48])
@pytest.mark.parametrize("n", [1, 65, 4097])
def test_permute_gathers_and_scatters(pkg, ctx, n, elem):
    rng = np.random.RandomState(n + elem)
    src = rng.randint(0, 256, (n, elem)).astype(np.uint8)
    order = rng.permutation(n).astype(np.uint32)
    d_src, d_order, d_mid, d_back = Dev(pkg, ctx, src), Dev(pkg, ctx, order), Dev(pkg, ctx, nbytes=n * elem), Dev(pkg, ctx, nbytes=n * elem)
    try:
        ctx.permute_device(d_src.ptr, d_mid.ptr, d_order.ptr, n, elem, scatter=False)
        ctx.permute_device(d_mid.ptr, d_back.ptr, d_order.ptr, n, elem, scatter=True)
        assert np.array_equal(d_mid.get().reshape(n, elem), src[order])       # gather: numpy's fancy indexing
        assert np.array_equal(d_back.get().reshape(n, elem), src)             # then scatter: the identity
    finally:
        for d in (d_src, d_order, d_mid, d_back):
            d.free()


def shuffled_with_invalid(pkg, rays, keys, seed):
    """The batch shuffled, one invalid ray of each kind interleaved (with keys of their own for the sampled forms)."""
    rng = np.random.RandomState(seed)
    perm = rng.permutation(rays.size)
    bad = invalid_rays(pkg)
    at = np.sort(rng.permutation(rays.size)[:len(bad)])
    r = np.insert(rays[perm], at, bad)
    k = None if keys is None else np.insert(keys[perm], at, rng.randint(0, 2 ** 32, len(bad), dtype=np.uint64).astype(np.uint32))
    return r, k


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("tag", ["p4_240x135", "teapot2_240x135"])
def test_sorted_queries_and_batches_equal_unsorted(pkg, golden, tag):
    scene = golden(tag).scene(pkg)
    c = pkg.Context(0)
    try:
        c.upload(scene)
        frame = pkg.frame_setup(scene.desc.camera, 160, 90)
        rays, _ = shuffled_with_invalid(pkg, pkg.camera_rays(frame), None, 1)
        eye = tuple(frame.cam_pos)
        hits = c.trace_rays(rays)
        assert (hits["flags"] & pkg.RTU_RAY_INVALID != 0).sum() == 7 and (hits["flags"] & pkg.RTU_RAY_HIT != 0).sum() > 1000
        assert same_bytes(c.trace_rays(rays, sort=True), hits)
        assert same_bytes(c.trace_rays(rays, sort=True, reference_walk=True), hits)
        occ = c.occluded(rays)
        assert same_bytes(c.occluded(rays, sort=True), occ) and same_bytes(c.occluded_rays(rays, sort=True), occ) and occ.sum() > 1000
        rgbt = c.shade_rays(rays, eye)[0]
        got = c.shade_rays(rays, eye, sort=True)[0]
        c.frame_status()  # complete
        assert same_bytes(got, rgbt)
        assert c.trace_rays(rays[:0], sort=True).size == 0 and c.shade_rays(rays[:0], eye, sort=True)[0].shape == (0, 4)
        with pytest.raises(pkg.RtuError):
            c.shade_rays(rays, eye, sort=True, stats=True)
    finally:
        c.close()


@pytest.mark.parametrize("tag,paths", [("p10_s4_160x120", False), ("p11_p2_120x68", True)], ids=["S-p10", "P-p11"])
def test_sorted_sampled_batches_equal_unsorted(pkg, golden, tag, paths):
    g = golden(tag)
    scene = g.scene(pkg)
    c = pkg.Context(0)
    try:
        c.upload(scene)
        frame = pkg.frame_setup(scene.desc.camera, g.width, g.height, samples=1, gather_bounces=4 if paths else 0)
        rays, keys = shuffled_with_invalid(pkg, *pkg.camera_sample_rays(frame, 0), 2)
        eye = tuple(frame.cam_pos)
        shade = c.shade_rays_paths if paths else c.shade_rays_sampled
        want = shade(rays, keys, eye)[0]
        got = shade(rays, keys, eye, sort=True)[0]
        c.frame_status()  # complete
        assert same_bytes(got, want) and (want[:, 3] < BIG).sum() > 1000 and (want[:, 3] == 0).sum() == 7
    finally:
        c.close()


def test_box_and_orders_follow_scene_changes(pkg, teapot):
    c, fresh = pkg.Context(0), pkg.Context(0)
    try:
        c.upload(teapot)
        box0 = c.ray_sort_box()
        assert same_bytes(box0, pkg.scene_sort_box(teapot))
        frame = pkg.frame_setup(teapot.desc.camera, 160, 90)
        rays, _ = shuffled_with_invalid(pkg, pkg.camera_rays(frame), None, 3)
        old_order = c.ray_order(rays)
        assert np.array_equal(old_order, expected(pkg, box0, rays)[1])
        moved = clone(pkg, teapot)
        moved.node_translate(1, (-3.0, 2.0, 9.0))
        c.update(moved)
        fresh.upload(moved)
        box1 = c.ray_sort_box()
        assert same_bytes(box1, fresh.ray_sort_box()) and same_bytes(box1, pkg.scene_sort_box(moved)) and not same_bytes(box1, box0)
        grown = clone(pkg, moved)
        grown.set_mesh_vertices(0, (grown.mesh_vertices(0) * np.float32(3)).astype(np.float32))
        c.update_meshes(grown, [0])
        fresh.upload(grown)
        box2 = c.ray_sort_box()
        assert same_bytes(box2, fresh.ray_sort_box()) and same_bytes(box2, pkg.scene_sort_box(grown)) and not same_bytes(box2, box1)
        new_order = c.ray_order(rays)
        assert np.array_equal(new_order, expected(pkg, box2, rays)[1]) and np.array_equal(new_order, fresh.ray_order(rays))
        # the order of the scene as it was is still a permutation, and round-trips: gather, trace, scatter = the unsorted answer
        assert np.array_equal(np.sort(old_order), np.arange(rays.size))
        hits = c.trace_rays(rays)
        back = np.zeros_like(hits)
        back[old_order] = c.trace_rays(rays[old_order])
        assert same_bytes(back, hits) and same_bytes(c.trace_rays(rays, sort=True), hits)
    finally:
        c.close()
        fresh.close()


def test_ordering_has_no_side_effects(pkg, teapot):
    c = pkg.Context(0)
    try:
        c.upload(teapot)
        frame = pkg.frame_setup(teapot.desc.camera, 160, 90)
        sampled = pkg.frame_setup(teapot.desc.camera, 160, 90, samples=4)
        rays, _ = shuffled_with_invalid(pkg, pkg.camera_rays(frame), None, 4)
        before = c.render(frame)[0]
        session = c.progressive(sampled)
        session.advance(2)
        counts = c.frame_counts()
        d_rays, d_order = Dev(pkg, c, rays), Dev(pkg, c, nbytes=4 * rays.size)
        stream = pkg.hip.rtu_context_stream(c._h)
        c.ray_order_device(d_rays.ptr, rays.size, d_order.ptr, stream)
        first = d_order.get(np.uint32)
        assert pkg.hip.rtu_frame_status(c._h) == pkg.RTU_OK and c.frame_counts() == counts
        a0 = pkg.hip.rtu_debug_device_allocations()
        for _ in range(3):  # the same size again: the scratch is there
            c.ray_order_device(d_rays.ptr, rays.size, d_order.ptr, stream)
            assert d_order.get(np.uint32).tobytes() == first.tobytes()
        c.ray_order_device(d_rays.ptr, rays.size // 3, d_order.ptr, stream)  # and a smaller one
        assert pkg.hip.rtu_context_sync(c._h) == pkg.RTU_OK
        assert pkg.hip.rtu_debug_device_allocations() == a0
        assert pkg.hip.rtu_frame_status(c._h) == pkg.RTU_OK and c.frame_counts() == counts
        d_rays.free()
        d_order.free()
        assert same_bytes(c.render(frame)[0], before)
        # the open session goes on as if nothing had happened: it ends in the one-shot image
        session.advance(2)
        assert session.status()[0] == 4
        assert same_bytes(session.snapshot()[0], c.render(sampled)[0])
        session.close()
    finally:
        c.close()


def test_errors(pkg, ctx, p4):
    hip, ARG = pkg.hip, pkg.RTU_ERR_ARG
    rays = mixed_rays(pkg, ctx.ray_sort_box(), 64, 9)
    d_rays, d_order, d_out = Dev(pkg, ctx, rays), Dev(pkg, ctx, nbytes=4 * 64), Dev(pkg, ctx, nbytes=48 * 64)
    empty = pkg.Context(0)
    try:
        assert hip.rtu_frame_status(ctx._h) == pkg.RTU_OK
        box = np.zeros(6, np.float32)
        fp = box.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        order = np.zeros(64, np.uint32)
        # before an upload
        assert hip.rtu_ray_sort_box(empty._h, fp) == pkg.RTU_ERR_NO_SCENE
        assert hip.rtu_ray_order_device(empty._h, d_rays.ptr, 64, d_order.ptr, None) == pkg.RTU_ERR_NO_SCENE
        assert hip.rtu_ray_order(empty._h, rays.ctypes.data, 64, order.ctypes.data) == pkg.RTU_ERR_NO_SCENE
        assert hip.rtu_ray_sort_box(ctx._h, None) == ARG
        # rtu_ray_order_device
        assert hip.rtu_ray_order_device(ctx._h, d_rays.ptr, (1 << 26) + 1, d_order.ptr, None) == ARG
        assert hip.rtu_ray_order_device(ctx._h, None, 64, d_order.ptr, None) == ARG
        assert hip.rtu_ray_order_device(ctx._h, d_rays.ptr, 64, None, None) == ARG
        assert hip.rtu_ray_order_device(ctx._h, d_rays.ptr + 8, 32, d_order.ptr, None) == ARG     # rays not 16-byte aligned
        assert hip.rtu_ray_order_device(ctx._h, d_rays.ptr, 32, d_order.ptr + 2, None) == ARG     # order not 4-byte aligned
        assert hip.rtu_ray_order_device(ctx._h, None, 0, None, None) == pkg.RTU_OK                # n == 0: nothing is launched
        assert hip.rtu_ray_order(ctx._h, None, 64, order.ctypes.data) == ARG
        assert hip.rtu_ray_order(ctx._h, rays.ctypes.data, 64, None) == ARG
        assert hip.rtu_ray_order(ctx._h, rays.ctypes.data, (1 << 26) + 1, order.ctypes.data) == ARG
        assert hip.rtu_ray_order(ctx._h, None, 0, None) == pkg.RTU_OK
        assert ctx.ray_order(rays[:0]).size == 0
        # rtu_permute_device
        for elem in (0, 2, 3, 8, 12, 24, 64):
            assert hip.rtu_permute_device(ctx._h, d_rays.ptr, d_out.ptr, d_order.ptr, 8, elem, 0, None) == ARG
        assert hip.rtu_permute_device(ctx._h, d_rays.ptr, d_out.ptr, d_order.ptr, 8, 32, 2, None) == ARG   # scatter is 0 or 1
        assert hip.rtu_permute_device(ctx._h, d_rays.ptr, d_rays.ptr, d_order.ptr, 8, 32, 0, None) == ARG  # in place
        assert hip.rtu_permute_device(ctx._h, None, d_out.ptr, d_order.ptr, 8, 32, 0, None) == ARG
        assert hip.rtu_permute_device(ctx._h, d_rays.ptr, None, d_order.ptr, 8, 32, 0, None) == ARG
        assert hip.rtu_permute_device(ctx._h, d_rays.ptr, d_out.ptr, None, 8, 32, 0, None) == ARG
        assert hip.rtu_permute_device(ctx._h, d_rays.ptr + 4, d_out.ptr, d_order.ptr, 8, 16, 0, None) == ARG
        assert hip.rtu_permute_device(ctx._h, d_rays.ptr, d_out.ptr + 2, d_order.ptr, 8, 4, 0, None) == ARG
        assert hip.rtu_permute_device(ctx._h, d_rays.ptr, d_out.ptr, d_order.ptr + 1, 8, 1, 0, None) == ARG
        assert hip.rtu_permute_device(ctx._h, d_rays.ptr, d_out.ptr, d_order.ptr, (1 << 26) + 1, 1, 0, None) == ARG
        assert hip.rtu_permute_device(ctx._h, None, None, None, 0, 4, 0, None) == pkg.RTU_OK
        assert hip.rtu_permute_device(empty._h, None, None, None, 0, 4, 0, None) == pkg.RTU_OK  # needs no scene
        assert hip.rtu_frame_status(ctx._h) == pkg.RTU_OK  # no refusal left a trace
        assert np.array_equal(order_device(pkg, ctx, rays), expected(pkg, ctx.ray_sort_box(), rays)[1])  # and it still works
    finally:
        for d in (d_rays, d_order, d_out):
            d.free()
        empty.close()
