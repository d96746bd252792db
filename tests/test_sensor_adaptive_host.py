"""Adaptive sensors (include/rtu_render.h, "Adaptive sensors"), the part that needs no GPU: the symbols, the refusals that need no
device, and the link to the oracle — on p4 the oracle shades sensor_rays(desc, k) of every sample, the rule is replayed in numpy on
what it answers, and the counts, the margins and the per-sample images are kept for tests/test_gpu_sensor_adaptive.py.

The margin of a pixel is the project's (tests/test_gpu_adaptive_oracle.py): the smallest relative distance between its largest channel
variance and the target over the checkpoints the rule evaluated up to its stop. A pixel with a margin below 1e-3 is borderline: the
device may decide it either way through the last bit of a sample. The borderline pixels are at most 0.1 % of an image — a cap on what a
comparison may leave out, not a tolerance."""
import ctypes

import numpy as np
import pytest

from test_gpu_adaptive import replay
from test_sensor_host import BIG, make, refusals, scene_sensors

f32 = np.float32
SYMBOLS = ("rtu_render_sensor_adaptive", "rtu_render_sensor_adaptive_device", "rtu_debug_sensor_adaptive_trace")
# name -> (index into scene_sensors, samples, min_samples, increment)
ORACLE_CASES = {"ortho": (1, 12, 4, 2), "equirect": (0, 17, 3, 1)}
# the count maps of the two cases, measured on the oracle alone with middle_target
EXPECTED_COUNTS = {"ortho": {4: 2155, 6: 6, 8: 4, 10: 2, 12: 137}, "equirect": {3: 2004, 15: 1, 17: 43}}
_cache = {}


def test_symbols(pkg):
    for s in SYMBOLS:
        assert s in pkg.HIP_SYMBOLS and hasattr(pkg.hip, s)
    assert callable(pkg.Context.render_sensor_adaptive) and callable(pkg.Context.render_sensor_adaptive_device)
    assert callable(pkg.Context.sensor_adaptive_trace)


def adaptive_violations(pkg, samples):
    """(what, an RtuAdaptiveDesc that breaks that one rule) for a sensor of `samples` samples."""
    ok = dict(min_samples=2)
    return [(str(kw), pkg.adaptive_defaults(**dict(ok, **kw)))
            for kw in ({"min_samples": 0}, {"min_samples": samples + 1}, {"increment": 0}, {"increment": -2}, {"target_variance": float("nan")},
                       {"target_variance": -1e-6}, {"max_batch": -1}, {"max_batch": pkg.RTU_MAX_BATCH + 1})]


def test_refusals_without_a_device(pkg):
    """A NULL context never reaches a GPU, whatever comes with it."""
    hip = pkg.hip
    out, counts = np.zeros((4, 8, 4), f32), np.zeros((4, 8), np.uint8)
    ok, ad = make(pkg, "equirect", 8, 4, 4), pkg.adaptive_defaults(min_samples=2)

    def host(d, a):
        return hip.rtu_render_sensor_adaptive(None, ctypes.byref(d) if d is not None else None, ctypes.byref(a) if a is not None else None,
                                              out.ctypes.data, counts.ctypes.data)

    def device(d, a):
        return hip.rtu_render_sensor_adaptive_device(None, ctypes.byref(d) if d is not None else None, ctypes.byref(a) if a is not None else None,
                                                     8192, None, None)
    cases = [("ok", ok, ad), ("no sensor", None, ad), ("no adaptive", ok, None)]
    cases += [(what, d, ad) for what, d in refusals(pkg)]
    cases += [("samples %d" % s, make(pkg, "equirect", 8, 4, s), pkg.adaptive_defaults(min_samples=1)) for s in (0, 256)]
    cases += [(what, ok, a) for what, a in adaptive_violations(pkg, 4)]
    assert len(cases) == 3 + 36 + 2 + 8
    for what, d, a in cases:
        assert host(d, a) == pkg.RTU_ERR_ARG and device(d, a) == pkg.RTU_ERR_ARG, what
    assert not out.any() and not counts.any()
    live = (ctypes.c_uint32 * 4)()
    assert hip.rtu_debug_sensor_adaptive_trace(None, live, live, 4) == pkg.RTU_ERR_ARG


# ---- the oracle link --------------------------------------------------------------------------------------------------------------
def checkpoint_variances(imgs, min_samples, increment):
    """[(n, the largest channel variance at n)] for every checkpoint n = min_samples + k * increment < samples: the rule's expression."""
    S = imgs.shape[0]
    s = np.zeros(imgs.shape[1:3] + (3,), f32)
    q = np.zeros_like(s)
    out = []
    for i in range(S):
        x = imgs[i, ..., :3]
        s = s + x
        q = q + x * x
        n = i + 1
        if n < S and n >= min_samples and (n - min_samples) % increment == 0:
            var = np.full(s.shape, np.inf, f32) if n == 1 else (q - s * (s / f32(n))) / f32(n - 1)
            out.append((n, var.max(axis=-1)))
    return out


def middle_target(imgs, min_samples):
    """The geometric mean of the two middle values of the sorted distinct non-zero largest-channel variances at min_samples."""
    v = checkpoint_variances(imgs[:min_samples + 1], min_samples, 1)[0][1]
    u = np.unique(v[(v > 0) & np.isfinite(v)]).astype(np.float64)
    assert u.size >= 2
    return float(f32(np.sqrt(u[u.size // 2 - 1] * u[u.size // 2])))


def margins(imgs, min_samples, increment, target, counts):
    """Per pixel the smallest |var - target| / target over the checkpoints n <= its count (a pixel that stopped at samples saw all)."""
    m = np.full(imgs.shape[1:3], np.inf, np.float64)
    for n, v in checkpoint_variances(imgs, min_samples, increment):
        seen = counts >= n
        with np.errstate(invalid="ignore"):
            rel = np.abs(v.astype(np.float64) - target) / target
        m = np.where(seen, np.minimum(m, np.where(np.isnan(rel), np.inf, rel)), m)
    return m


def oracle_case(pkg, orc, golden, name):
    """The oracle's side of a case of ORACLE_CASES, computed once per process: dict(scene, desc, adaptive, imgs [S, H, W, 4] — per
    sample what the sensor accumulator adds, a miss with t = RTU_BIGFLOAT —, target, image, counts, margin)."""
    if name in _cache:
        return _cache[name]
    which, S, mn, inc = ORACLE_CASES[name]
    scene = golden("p4_240x135").scene(pkg)
    base = scene_sensors(pkg, scene)[which]
    d = pkg.RtuSensorDesc.from_buffer_copy(bytes(base))
    d.samples = S
    imgs = np.empty((S, d.height, d.width, 4), f32)
    for k in range(S):
        rays, _ = pkg.sensor_rays(d, k)
        out, _ = orc.shade_rays(scene, rays, eye=tuple(d.pos), threads=8, max_bounce=d.max_bounce)
        assert (out[:, 3] > 0).all()  # every ray of these two sensors is valid
        imgs[k] = out.reshape(d.height, d.width, 4)
    target = middle_target(imgs, mn)
    image, counts = replay(imgs, mn, inc, target)
    case = dict(scene=scene, desc=d, adaptive=pkg.adaptive_defaults(min_samples=mn, increment=inc, target_variance=target), imgs=imgs, target=target,
                image=image, counts=counts, margin=margins(imgs, mn, inc, target, counts))
    imgs.setflags(write=False)
    _cache[name] = case
    return case


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_oracle_replay(pkg, orc, golden, name):
    c = oracle_case(pkg, orc, golden, name)
    _, S, mn, inc = ORACLE_CASES[name]
    values, n = np.unique(c["counts"], return_counts=True)
    hist = dict(zip(values.tolist(), n.tolist()))
    border = c["margin"] < 1e-3
    print("p4 %s %dx%d, %d / %d / %d, target %.9g: counts %s, %d borderline" % (name, c["desc"].width, c["desc"].height, S, mn, inc, c["target"], hist,
                                                                               int(border.sum())))
    assert min(hist) == mn and max(hist) == S
    if name == "ortho":
        assert len(hist) >= 3
    assert border.sum() <= 1e-3 * border.size
    assert hist == EXPECTED_COUNTS[name]
    assert (c["imgs"][..., 3] != BIG).any() and (c["imgs"][..., 3] == BIG).any()  # hits and misses
