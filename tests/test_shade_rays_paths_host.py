"""Path-traced ray batches (rtu_shade_rays_paths, include/rtu_render.h), the part that needs no GPU: the two symbols, their
bindings, and the NULL-context / NULL-descriptor answers."""
import ctypes

import numpy as np


def test_the_library_exports_the_two_symbols(pkg):
    for name in ("rtu_shade_rays_paths_device", "rtu_shade_rays_paths"):
        assert hasattr(pkg.hip, name), "librtu_hip.so does not export " + name
        assert name in pkg.HIP_SYMBOLS
    assert callable(pkg.Context.shade_rays_paths) and callable(pkg.Context.shade_rays_paths_device)


def test_a_null_context_or_descriptor_is_an_argument_error(pkg):
    rays = np.zeros(4, pkg.ray_dtype())
    keys = np.zeros(4, np.uint32)
    out = np.zeros((4, 4), np.float32)
    d = pkg.shade_desc()
    hip = pkg.hip
    assert hip.rtu_shade_rays_paths(None, rays.ctypes.data, keys.ctypes.data, 4, ctypes.byref(d), out.ctypes.data, None) == pkg.RTU_ERR_ARG
    assert hip.rtu_shade_rays_paths_device(None, 16, 16, 4, ctypes.byref(d), 16, None) == pkg.RTU_ERR_ARG
    assert hip.rtu_shade_rays_paths(None, None, None, 0, ctypes.byref(d), None, None) == pkg.RTU_ERR_ARG
    assert hip.rtu_shade_rays_paths_device(None, None, None, 0, None, None, None) == pkg.RTU_ERR_ARG
    assert hip.rtu_shade_rays_paths(None, rays.ctypes.data, keys.ctypes.data, 4, None, out.ctypes.data, None) == pkg.RTU_ERR_ARG
    assert hip.rtu_shade_rays_paths_device(None, 16, 16, 4, None, 16, None) == pkg.RTU_ERR_ARG
