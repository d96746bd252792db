"""GPU: the denoising filter's device form (rtu_denoise_device) against its host form (rtu_denoise, which tests/test_denoise_host.py
holds to the rules), bit for bit — on the synthetic inputs of that file and on real recipe-P snapshots with the features of
rtu_frame_features —, and the denoised snapshot of a progressive session (rtu_progressive_snapshot_denoised)."""
import ctypes

import numpy as np
import pytest

from test_denoise_host import SIZES, inputs_ok, make_inputs
from test_gpu_ray_query import bits, materials
from test_mesh_update_host import clone

pytestmark = pytest.mark.gpu

F = np.float32
TAG = "p11_p2_120x68"
DESCS = [{}, {"n_passes": 1}, {"n_passes": 2}, {"n_passes": 6}, {"n_passes": 8, "sigma_color": 0.35, "sigma_plane": 0.2, "normal_log2_power": 0},
         {"n_passes": 3, "normal_log2_power": 7}]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def device_denoise(pkg, ctx, rgbz, hits, albedo, desc, in_place=False, stream=None):
    import torch
    H, W = rgbz.shape[:2]
    d = pkg.denoise_desc(W, H)
    ctypes.memmove(ctypes.byref(d), ctypes.byref(desc), ctypes.sizeof(d))
    d.width, d.height = W, H
    d_in = torch.from_numpy(np.ascontiguousarray(rgbz).view(np.uint8).copy()).to("cuda:0")
    d_hits = torch.from_numpy(np.ascontiguousarray(hits).view(np.uint8).copy()).to("cuda:0")
    d_alb = torch.from_numpy(np.ascontiguousarray(albedo).view(np.uint8).copy()).to("cuda:0")
    d_out = d_in if in_place else torch.full((H * W * 16,), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.denoise_device(d, d_in.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_out.data_ptr(), stream.cuda_stream if stream else None)
    (stream or torch.cuda).synchronize()
    if not in_place:
        assert np.array_equal(d_in.cpu().numpy().reshape(-1), np.ascontiguousarray(rgbz).view(np.uint8).reshape(-1)), "the input was written"
    return d_out.cpu().numpy().view(F).reshape(H, W, 4)


# ---- 7. the device form against the host form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES + [(200, 150)], ids=lambda s: "%dx%d" % s)
def test_device_form_equals_the_host_form(pkg, ctx, size):
    import torch
    rgbz, hits, albedo = make_inputs(pkg, size[0], size[1], 1234 + (SIZES + [(200, 150)]).index(size))
    inputs_ok(rgbz, hits, albedo)
    stream = torch.cuda.Stream(device=0)
    for k, over in enumerate(DESCS):
        desc = pkg.denoise_desc(**over)
        want = pkg.denoise(rgbz, hits, albedo, desc)
        got = device_denoise(pkg, ctx, rgbz, hits, albedo, desc, stream=stream if k % 2 else None)
        diff = bits(got) != bits(want)
        assert not diff.any(), "%s: %d words differ, first at %s" % (over, diff.sum(), np.argwhere(diff)[0])
        same = device_denoise(pkg, ctx, rgbz, hits, albedo, desc, in_place=True)
        assert np.array_equal(bits(same), bits(want)), "%s: d_out == d_in gives other bits" % over
        if size != (1, 1):
            assert (bits(want) != bits(rgbz)).any()


@pytest.fixture(scope="module")
def room(pkg, golden, ctx):
    """p11_p2_120x68: the scene, its recipe-P frame of 4 samples, the features of the frame; made once and left unchanged."""
    g = golden(TAG)
    scene = g.scene(pkg)
    frame = pkg.frame_setup(scene.desc.camera, g.width, g.height, samples=4, gather_bounces=4)
    ctx.upload(scene)
    hits, albedo = ctx.frame_features(frame)
    for a in (hits, albedo):
        a.setflags(write=False)
    return scene, frame, hits, albedo


def test_real_snapshots_with_frame_features(pkg, ctx, room):
    scene, frame, hits, albedo = room
    ctx.upload(scene)
    assert ((hits["flags"] & 1) != 0).all() and albedo[:, :3].any(), "a closed room: every pixel has a guide"
    s = ctx.progressive(frame)
    try:
        for n in (1, 1, 2):  # snapshots at 1, 2 and 4 samples
            s.advance(n)
            snap = s.snapshot()[0]
            for over in ({}, {"n_passes": 3}):
                desc = pkg.denoise_desc(**over)
                want = pkg.denoise(snap, hits, albedo, desc)
                got = device_denoise(pkg, ctx, snap, hits, albedo, desc)
                assert np.array_equal(bits(got), bits(want)), "%d samples %s" % (s.status()[0], over)
                assert (bits(want[..., :3]) != bits(snap[..., :3])).any() and np.array_equal(bits(want[..., 3]), bits(snap[..., 3]))
    finally:
        s.close()


# ---- 8. progressive sessions -----------------------------------------------------------------------------------------------------------
def test_progressive_snapshot_denoised(pkg, ctx, room):
    import torch
    scene, frame, hits, albedo = room
    ctx.upload(scene)
    one_shot = ctx.render(frame)[0]
    s = ctx.progressive(frame)
    try:
        with pytest.raises(pkg.RtuError) as e:   # no samples yet
            s.snapshot_denoised()
        assert e.value.code == pkg.RTU_ERR_ARG
        s.advance(1)
        snap = s.snapshot()[0]
        first = s.snapshot_denoised()            # makes the session's features and the context's planes
        assert np.array_equal(bits(first), bits(pkg.denoise(snap, hits, albedo)))
        a0 = pkg.hip.rtu_debug_device_allocations()
        again = s.snapshot_denoised()
        assert pkg.hip.rtu_debug_device_allocations() == a0, "the second call allocated"
        assert np.array_equal(bits(again), bits(first))
        assert np.array_equal(bits(s.snapshot()[0]), bits(snap)), "the sums were touched"
        s.advance(1)
        desc = pkg.denoise_desc(n_passes=3, sigma_color=0.5)
        desc.width, desc.height = 5, 3           # ignored: the frame's are used
        snap2 = s.snapshot()[0]
        want2 = pkg.denoise(snap2, hits, albedo, desc)
        assert np.array_equal(bits(s.snapshot_denoised(desc)), bits(want2))
        d_out = torch.zeros((frame.height, frame.width, 4), dtype=torch.float32, device="cuda:0")
        stream = torch.cuda.Stream(device=0)
        torch.cuda.synchronize()
        a0 = pkg.hip.rtu_debug_device_allocations()
        s.snapshot_denoised_device(d_out.data_ptr(), desc, stream.cuda_stream)
        stream.synchronize()
        assert pkg.hip.rtu_debug_device_allocations() == a0
        assert np.array_equal(bits(d_out.cpu().numpy()), bits(want2))
        for bad in ({"n_passes": 0}, {"n_passes": 9}, {"sigma_plane": 0.0}):
            with pytest.raises(pkg.RtuError) as e:
                s.snapshot_denoised(pkg.denoise_desc(**bad))
            assert e.value.code == pkg.RTU_ERR_ARG
        s.advance(2)                             # driven to S: still the one-shot render
        assert np.array_equal(bits(s.snapshot()[0]), bits(one_shot))
        assert np.array_equal(bits(s.snapshot_denoised()), bits(pkg.denoise(one_shot, hits, albedo)))
    finally:
        s.close()
    # a sharded session is refused
    sharded = pkg.frame_setup(scene.desc.camera, frame.width, frame.height, shard_rank=0, shard_count=2, samples=2, gather_bounces=4)
    s = ctx.progressive(sharded)
    try:
        s.advance(1)
        with pytest.raises(pkg.RtuError) as e:
            s.snapshot_denoised()
        assert e.value.code == pkg.RTU_ERR_ARG
    finally:
        s.close()


def test_progressive_stale_rules(pkg, room):
    scene, frame, hits, albedo = room
    c = pkg.Context(0)
    try:
        c.upload(scene)
        holds, bare = c.progressive(frame), c.progressive(frame)
        holds.advance(1)
        bare.advance(1)
        before = holds.snapshot_denoised()       # `holds` has its features now, `bare` has none
        assert np.array_equal(bits(before), bits(pkg.denoise(holds.snapshot()[0], hits, albedo)))
        painted = clone(pkg, scene)
        for m in range(painted.desc.n_materials):
            materials(painted)[m].diffuse[0] = 0.9
        c.update(painted)
        with pytest.raises(pkg.RtuError) as e:
            holds.advance(1)
        assert e.value.code == pkg.RTU_ERR_STALE
        assert np.array_equal(bits(holds.snapshot_denoised()), bits(before)), "a stale session answers from the features it holds"
        with pytest.raises(pkg.RtuError) as e:
            bare.snapshot_denoised()
        assert e.value.code == pkg.RTU_ERR_STALE
        assert bare.snapshot()[0].shape == before.shape  # the plain snapshot still answers
        holds.close()
        bare.close()
    finally:
        c.close()


# ---- 9. argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors(pkg, ctx):
    import torch
    W, H = 7, 5
    n = W * H
    buf = torch.zeros(n * 16 + n * 48 + n * 16 + n * 16 + 64, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    assert base % 16 == 0
    ptrs = [base, base + n * 16, base + n * 64, base + n * 80]  # in, hits, albedo, out
    hip = pkg.hip

    def call(desc, p=ptrs):
        return hip.rtu_denoise_device(ctx._h, ctypes.byref(desc) if desc is not None else None, p[0], p[1], p[2], p[3], None)
    assert call(pkg.denoise_desc(W, H)) == pkg.RTU_OK
    for bad in ({"n_passes": 0}, {"n_passes": 9}, {"sigma_color": 0.0}, {"sigma_color": -1.0}, {"sigma_plane": 0.0}, {"sigma_plane": float("nan")},
                {"normal_log2_power": -1}, {"normal_log2_power": 8}, {"width": 0}, {"height": -3}):
        d = pkg.denoise_desc(W, H)
        for k, v in bad.items():
            setattr(d, k, v)
        assert call(d) == pkg.RTU_ERR_ARG, bad
    for k in range(2):
        d = pkg.denoise_desc(W, H)
        d.reserved[k] = 1
        assert call(d) == pkg.RTU_ERR_ARG
    assert call(None) == pkg.RTU_ERR_ARG
    for k in range(4):
        p = list(ptrs)
        p[k] = None
        assert call(pkg.denoise_desc(W, H), p) == pkg.RTU_ERR_ARG
        p[k] = ptrs[k] + 8  # not 16-byte aligned
        assert call(pkg.denoise_desc(W, H), p) == pkg.RTU_ERR_ARG
    assert hip.rtu_denoise_device(None, ctypes.byref(pkg.denoise_desc(W, H)), *ptrs, None) == pkg.RTU_ERR_ARG
    torch.cuda.synchronize()
