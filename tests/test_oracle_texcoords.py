"""The restatements of glibc's asinf, atanf and atan2f (oracle/rtu_oracle.cpp; the device's copy is in
raytracer-utah_amd/csrc/rtu_intersect.h) against the host libm, which the reference and recipe W call.

Exhaustive where it can be: every float for asinf on [-1, 1] and for atanf, 2^32 pairs for atan2f, threaded inside the
oracle library. A failure here means either a wrong restatement or a host libm whose algorithm is no longer the one
restated (glibc 2.35's fdlibm-derived binary32 code): the goldens and the device would then disagree with the host."""
import math
import os

import numpy as np
import pytest

THREADS = max(1, min(16, len(os.sched_getaffinity(0))))
CHANGED = ("the host libm differs from the restatement of glibc's binary32 %s: if the host glibc changed, the device's "
           "copy (rtu_intersect.h) no longer reproduces the libm the reference calls")


def _check(orc, fn, first, count, name, seed=0):
    bad, at = orc.check_portable(fn, first, count, seed, THREADS)
    assert bad == 0, (CHANGED % name) + ": %d of %d inputs, first at bits %08x %08x" % (bad, count, at[0], at[1])


@pytest.mark.parametrize("sign", [0, 0x80000000])
def test_asinf_every_float(orc, sign):
    """Every float of [0, 1] and of [-1, -0]: 2 x 1 065 353 217 inputs."""
    _check(orc, orc.FN_ASINF, sign, 0x3f800001, "asinf")


def test_atanf_every_float(orc):
    """All 2^32 bit patterns, NaNs and infinities included."""
    _check(orc, orc.FN_ATANF, 0, 1 << 32, "atanf")


def test_atan2f_pairs(orc):
    """2^32 pairs: any bit patterns, unit-vector components, near-diagonals, exponents within 70 of each other."""
    _check(orc, orc.FN_ATAN2F, 0, 1 << 32, "atan2f", seed=0x5eed)


def test_atan2f_special_cases(orc):
    """Every pair of signed zeros, infinities, NaN, axes, subnormals and the |y/x| = 2^+-60 cut-offs."""
    v = np.array([0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, 1e-40, 1.17549435e-38, -2.0, 0.5, 0.70710677, -0.70710677, 0.4375,
                  1.1875, 2.4375, 2 ** 25, -2 ** 25, 2 ** 60, 2 ** -60, 2 ** 61, 2 ** -61, 3e38, -3e38, math.inf, -math.inf,
                  math.nan], np.float32)
    a, b = np.meshgrid(v, v, indexing="ij")
    pairs = np.stack([a.ravel(), b.ravel()], axis=1)
    for fn, x in ((orc.FN_ATAN2F, pairs), (orc.FN_ASINF, v), (orc.FN_ATANF, v)):
        p, h = orc.libm(fn, x, True), orc.libm(fn, x, False)
        same = (p.view(np.uint32) == h.view(np.uint32)) | (np.isnan(p) & np.isnan(h))
        assert same.all(), "fn %d: %s" % (fn, x.reshape(len(p), -1)[~same][:8])


def test_oracle_texcoords_follow_x86_casts(orc):
    """The oracle's TileClamp is the reference's on x86: int(float) is INT_MIN for NaN and out of range, so 3e9 becomes
    3e9 + 2^31 (a saturating conversion would give 3e9 - 2^31), and -0 stays -0."""
    x = np.array([[3e9, -3e9, -0.0], [math.nan, 1e20, -1e-8]], np.float32)
    out = orc.texcoords(orc.TEXOP_TILE_CLAMP, x)
    assert out[0, 0] == np.float32(3e9) + np.float32(2 ** 31)
    assert out[0, 1] == np.float32(-3e9) + np.float32(2 ** 31)
    assert out[0, 2] == 0 and math.copysign(1, out[0, 2]) == -1
    assert np.isnan(out[1, 0]) and out[1, 1] == np.float32(1e20) and out[1, 2] == np.float32(1.0)


def test_oracle_texcoords_refuse_what_is_not_there(pkg, orc, golden, tmp_path):
    """TEXTURE / MAP need a textured scene and a present map; otherwise an argument error, never a read (the device's
    rtu_debug_texcoords refuses the same inputs: tests/test_gpu_texcoords.py)."""
    from test_gpu_texcoords import _present_maps, _texture_scene
    x = np.zeros((4, 3), np.float32)
    plain = golden("teapot2_240x135").scene(pkg)
    for op, index in ((orc.TEXOP_MAP, -1), (orc.TEXOP_MAP, -2), (orc.TEXOP_MAP, 0), (orc.TEXOP_TEXTURE, 0)):
        with pytest.raises(orc.OracleError) as e:
            orc.texcoords(op, x, index, plain)
        assert e.value.code == orc.ERR_ARG
    scene = _texture_scene(pkg, tmp_path)
    for i, present in _present_maps(pkg, scene).items():
        if present:
            assert orc.texcoords(orc.TEXOP_MAP, x, i, scene).shape == (4, 3)
        else:
            with pytest.raises(orc.OracleError):
                orc.texcoords(orc.TEXOP_MAP, x, i, scene)
