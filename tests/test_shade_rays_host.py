"""Ray batches (rtu_shade_rays, include/rtu_render.h), the part that needs no GPU: the three symbols, the descriptor's layout and
defaults, and the NULL-context answers."""
import ctypes

import numpy as np


def test_the_library_exports_the_three_symbols(pkg):
    for name in ("rtu_shade_defaults", "rtu_shade_rays_device", "rtu_shade_rays"):
        assert hasattr(pkg.hip, name), "librtu_hip.so does not export " + name
        assert name in pkg.HIP_SYMBOLS


def test_shade_defaults_writes_exactly_32_bytes(pkg):
    assert ctypes.sizeof(pkg.RtuShadeDesc) == 32
    assert pkg.RtuShadeDesc.max_bounce.offset == 12 and pkg.RtuShadeDesc.flags.offset == 16 and pkg.RtuShadeDesc.reserved.offset == 20
    buf = np.full(96, 0xA5, np.uint8)  # 32 guard bytes in front of the struct, 32 behind it
    d = pkg.RtuShadeDesc.from_buffer(buf, 32)
    assert pkg.hip.rtu_shade_defaults(ctypes.byref(d)) == pkg.RTU_OK
    assert np.all(buf[:32] == 0xA5) and np.all(buf[64:] == 0xA5)
    assert list(d.eye) == [0.0, 0.0, 0.0] and d.max_bounce == 5 and d.flags == 0 and list(d.reserved) == [0, 0, 0]
    want = np.zeros(32, np.uint8)
    want[12] = 5
    assert np.array_equal(buf[32:64], want)
    assert pkg.hip.rtu_shade_defaults(None) == pkg.RTU_ERR_ARG


def test_shade_desc_helper(pkg):
    d = pkg.shade_desc((1.0, -2.0, 3.5), max_bounce=2, reference_walk=True)
    assert list(d.eye) == [1.0, -2.0, 3.5] and d.max_bounce == 2 and d.flags == pkg.RTU_QUERY_REFERENCE_WALK and list(d.reserved) == [0, 0, 0]


def test_a_null_context_is_an_argument_error(pkg):
    rays = np.zeros(4, pkg.ray_dtype())
    out = np.zeros((4, 4), np.float32)
    d = pkg.shade_desc()
    assert pkg.hip.rtu_shade_rays(None, rays.ctypes.data, 4, ctypes.byref(d), out.ctypes.data, None) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_shade_rays_device(None, 16, 4, ctypes.byref(d), 16, None) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_shade_rays(None, None, 0, ctypes.byref(d), None, None) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_shade_rays_device(None, None, 0, None, None, None) == pkg.RTU_ERR_ARG
