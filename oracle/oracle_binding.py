"""ctypes view of oracle/librtu_oracle.so — TEST INFRASTRUCTURE.

May be imported only by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg. The product package never imports this module."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_PATH = os.path.join(_HERE, "librtu_oracle.so")
if not os.path.exists(_PATH):
    raise ImportError("%s missing: run `make -C oracle` (or __graft_entry__.build())" % _PATH)
lib = ctypes.CDLL(_PATH)

STAT_FIELDS = ("primary_rays", "primary_hits", "secondary_rays", "shadow_rays", "node_tests", "mesh_entries",
               "inner_visits", "leaf_visits", "leaf_elems", "tri_tests", "tri_accepts")
ERR_ARG, ERR_STOCHASTIC, ERR_UNSUPPORTED = -1, -2, -3


class OracleStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in STAT_FIELDS]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in STAT_FIELDS}


lib.rtu_oracle_render_rows.restype = ctypes.c_int
lib.rtu_oracle_render_rows.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.POINTER(OracleStats), ctypes.c_int]
lib.rtu_oracle_render.restype = ctypes.c_int
lib.rtu_oracle_render.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                  ctypes.POINTER(OracleStats), ctypes.c_int]
lib.rtu_oracle_render_scheduled.restype = ctypes.c_int
lib.rtu_oracle_render_scheduled.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
lib.rtu_oracle_camera_frame.restype = ctypes.c_int
lib.rtu_oracle_camera_frame.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
lib.rtu_oracle_postprocess.restype = None
lib.rtu_oracle_postprocess.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p]


lib.rtu_oracle_render_samples.restype = ctypes.c_int
lib.rtu_oracle_render_samples.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(OracleStats), ctypes.c_int]
lib.rtu_oracle_render_paths.restype = ctypes.c_int
lib.rtu_oracle_render_paths.argtypes = lib.rtu_oracle_render_samples.argtypes
lib.rtu_oracle_render_sample_images.restype = ctypes.c_int
lib.rtu_oracle_render_sample_images.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 8 + [ctypes.c_void_p, ctypes.c_int]
lib.rtu_oracle_render_adaptive.restype = ctypes.c_int
lib.rtu_oracle_render_adaptive.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 8 + [ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 4 +
                                           [ctypes.POINTER(OracleStats), ctypes.c_int])
lib.rtu_oracle_portable_acos.restype = None
lib.rtu_oracle_portable_acos.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
lib.rtu_oracle_portable_sincos.restype = None
lib.rtu_oracle_portable_sincos.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
for _n, _k in (("rtu_oracle_rand31", 2), ("rtu_oracle_sample_key", 2), ("rtu_oracle_child_key", 2)):
    getattr(lib, _n).restype = ctypes.c_uint32
    getattr(lib, _n).argtypes = [ctypes.c_uint32] * _k
lib.rtu_oracle_texcoords.restype = ctypes.c_int
lib.rtu_oracle_texcoords.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int]
for _n in ("rtu_oracle_portable_libm", "rtu_oracle_host_libm"):
    getattr(lib, _n).restype = None
    getattr(lib, _n).argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
lib.rtu_oracle_check_portable.restype = ctypes.c_longlong
lib.rtu_oracle_check_portable.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]
FN_ASINF, FN_ATANF, FN_ATAN2F = 0, 1, 2
STREAM_KEYED, STREAM_SEQUENTIAL = 0, 1
TRIG_PORTABLE, TRIG_LIBM = 0, 1


class OracleError(RuntimeError):
    def __init__(self, code):
        self.code = code
        super().__init__("oracle error %d" % code)


MAX_BOUNCE = 5  # RTU_MAX_BOUNCE: what the reference passes, and what the oracle is at between calls
lib.rtu_oracle_debug_max_bounce.restype = ctypes.c_int
lib.rtu_oracle_debug_max_bounce.argtypes = [ctypes.c_int]


class _bounces:
    """Test hook: the root Shade() calls of the renders inside the block receive bounceCount `max_bounce` (RtuFrameDesc.max_bounce
    of the device); the oracle is back at the reference's 5 afterwards, whatever happened."""

    def __init__(self, max_bounce):
        if not 0 <= int(max_bounce) <= MAX_BOUNCE:
            raise ValueError("max_bounce %r outside 0..%d" % (max_bounce, MAX_BOUNCE))
        self.k = int(max_bounce)

    def __enter__(self):
        lib.rtu_oracle_debug_max_bounce(self.k)

    def __exit__(self, *exc):
        lib.rtu_oracle_debug_max_bounce(MAX_BOUNCE)


def max_bounce_now():
    """The depth the oracle renders at (5 outside a call that was given another)."""
    return lib.rtu_oracle_debug_max_bounce(-1)


def render(scene, width, height, threads=1, row0=0, nrows=None, max_bounce=MAX_BOUNCE):
    """Recipe W. `scene` is a raytracer_utah_amd.Scene. Returns (rgbz [rows,W,4] float32, stats dict)."""
    if nrows is None:
        nrows = height - row0
    out = np.empty((nrows, width, 4), np.float32)
    st = OracleStats()
    with _bounces(max_bounce):
        rc = lib.rtu_oracle_render_rows(scene.desc_ptr, width, height, row0, nrows, out.ctypes.data, ctypes.byref(st), threads)
    if rc != 0:
        raise OracleError(rc)
    return out, st.as_dict()


def debug_all_triangles(on):
    """Test hook: the oracle tests every triangle of a mesh whatever its boxes say (not the reference's algorithm)."""
    lib.rtu_oracle_debug_all_triangles.argtypes = [ctypes.c_int]
    lib.rtu_oracle_debug_all_triangles.restype = None
    lib.rtu_oracle_debug_all_triangles(1 if on else 0)


def render_scheduled(scene, width, height, threads, per_pixel):
    """Recipe W, whole frame; per_pixel: the reference's PixelIterator schedule (one atomic fetch per pixel,
    PixelIterator.h:25-38) instead of chunks of rows. Same image, different scaling."""
    out = np.empty((height, width, 4), np.float32)
    st = OracleStats()
    rc = lib.rtu_oracle_render_scheduled(scene.desc_ptr, width, height, out.ctypes.data, ctypes.byref(st), threads, 1 if per_pixel else 0)
    if rc != 0:
        raise OracleError(rc)
    return out, st.as_dict()


def render_samples(scene, width, height, spp, stream=STREAM_KEYED, trig=TRIG_PORTABLE, threads=1, row0=0, nrows=None,
                   max_bounce=MAX_BOUNCE):
    """Recipe S (row f1): spp samples per pixel with soft shadows / glossy bounces / depth of field."""
    if nrows is None:
        nrows = height - row0
    out = np.empty((nrows, width, 4), np.float32)
    st = OracleStats()
    with _bounces(max_bounce):
        rc = lib.rtu_oracle_render_samples(scene.desc_ptr, width, height, row0, nrows, spp, stream, trig, out.ctypes.data,
                                           ctypes.byref(st), threads)
    if rc != 0:
        raise OracleError(rc)
    return out, st.as_dict()


def render_paths(scene, width, height, spp, stream=STREAM_KEYED, trig=TRIG_PORTABLE, threads=1, row0=0, nrows=None,
                 max_bounce=MAX_BOUNCE):
    """Recipe P (config 5): recipe S plus the 4-bounce Monte-Carlo gather."""
    if nrows is None:
        nrows = height - row0
    out = np.empty((nrows, width, 4), np.float32)
    st = OracleStats()
    with _bounces(max_bounce):
        rc = lib.rtu_oracle_render_paths(scene.desc_ptr, width, height, row0, nrows, spp, stream, trig, out.ctypes.data,
                                         ctypes.byref(st), threads)
    if rc != 0:
        raise OracleError(rc)
    return out, st.as_dict()


def sample_images(scene, width, height, spp, first, n, gi=False, threads=1, row0=0, nrows=None, max_bounce=MAX_BOUNCE):
    """Samples [first, first + n) of the fixed spp-sample frame of recipe S (gi False) or P (gi True), keyed stream, portable trig:
    float32 [n, rows, W, 4] {r, g, b, z}, z = RTU_BIGFLOAT for a miss (what rtu_debug_sample_images returns)."""
    if nrows is None:
        nrows = height - row0
    out = np.empty((n, nrows, width, 4), np.float32)
    with _bounces(max_bounce):
        rc = lib.rtu_oracle_render_sample_images(scene.desc_ptr, width, height, row0, nrows, spp, 1 if gi else 0, first, n, out.ctypes.data,
                                                 threads)
    if rc != 0:
        raise OracleError(rc)
    return out


def render_adaptive(scene, width, height, spp, min_samples, increment, target, gi=False, trace_batch=1, counts_in=None, threads=1,
                    row0=0, nrows=None, max_bounce=MAX_BOUNCE):
    """Adaptive recipe S / P as include/rtu_render.h states it (keyed stream, portable trig). Returns (rgbz float32 [rows, W, 4],
    counts uint8 [rows, W] — the rule's —, margin float32 [rows, W], stats dict). counts_in (uint8 [rows, W]): each pixel returns the
    mean of its first counts_in samples instead of the rule's. margin: the smallest |max var - target| over the checkpoints the
    rule evaluated up to its stop (relative to target when 0 < target < inf). trace_batch: a pixel stopped at n is traced on, for the
    counters only, to min(spp, trace_batch * ceil(n / trace_batch)), as the device does with batches of that size (1: nothing more)."""
    if nrows is None:
        nrows = height - row0
    out = np.empty((nrows, width, 4), np.float32)
    counts = np.empty((nrows, width), np.uint8)
    margin = np.empty((nrows, width), np.float32)
    cin = None
    if counts_in is not None:
        cin = np.ascontiguousarray(counts_in, np.uint8)
        if cin.shape != (nrows, width):
            raise ValueError("counts_in has shape %s, not %s" % (cin.shape, (nrows, width)))
    st = OracleStats()
    with _bounces(max_bounce):
        rc = lib.rtu_oracle_render_adaptive(scene.desc_ptr, width, height, row0, nrows, spp, 1 if gi else 0, min_samples, increment, target,
                                            trace_batch, cin.ctypes.data if cin is not None else None,
                                            out.ctypes.data, counts.ctypes.data, margin.ctypes.data, ctypes.byref(st), threads)
    if rc != 0:
        raise OracleError(rc)
    return out, counts, margin, st.as_dict()


def portable_acos(x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    lib.rtu_oracle_portable_acos(x.ctypes.data, x.size, out.ctypes.data)
    return out


def portable_sincos(t):
    t = np.ascontiguousarray(t, np.float32)
    s, c = np.empty_like(t), np.empty_like(t)
    lib.rtu_oracle_portable_sincos(t.ctypes.data, t.size, s.ctypes.data, c.ctypes.data)
    return s, c


def camera_frame(camera, width, height):
    out = np.empty(12, np.float32)
    rc = lib.rtu_oracle_camera_frame(ctypes.addressof(camera), width, height, out.ctypes.data)
    if rc != 0:
        raise OracleError(rc)
    return out.reshape(4, 3)  # pos, origin, u, v


def postprocess(rgbz):
    """gamma + Color24 + z-image: returns (rgb8 [H,W,3], z [H,W], zimg8 [H,W])."""
    a = np.ascontiguousarray(rgbz, np.float32)
    h, w = a.shape[:2]
    rgb = np.empty((h, w, 3), np.uint8)
    z = np.empty((h, w), np.float32)
    zi = np.empty((h, w), np.uint8)
    lib.rtu_oracle_postprocess(a.ctypes.data, w, h, rgb.ctypes.data, z.ctypes.data, zi.ctypes.data)
    return rgb, z, zi


# the op codes of rtu_oracle_texcoords are those of the device's rtu_debug_texcoords (TEXOP_* of the package)
TEXOP_ATAN2F, TEXOP_ASINF, TEXOP_SPHERE_UV, TEXOP_ENV_UVW, TEXOP_TILE_CLAMP, TEXOP_TEXTURE, TEXOP_MAP = range(7)
_TEXOP_IN = (2, 1, 3, 3, 3, 3, 3)
_TEXOP_OUT = (1, 1, 3, 3, 3, 3, 3)


def texcoords(op, x, index=0, scene=None, threads=8):
    """The oracle's texture arithmetic (libm atan2f / asinf, sphere uv, environment uvw, tile_clamp, texture_sample,
    map_sample) on the inputs x: float32 [n, out] (or [n]), the layout of the package's Context.texcoords."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    n = x.size // _TEXOP_IN[op]
    out = np.empty((n, _TEXOP_OUT[op]) if _TEXOP_OUT[op] > 1 else (n,), np.float32)
    rc = lib.rtu_oracle_texcoords(scene.desc_ptr if scene is not None else None, op, index, x.ctypes.data, n, out.ctypes.data, threads)
    if rc != 0:
        raise OracleError(rc)
    return out


def libm(fn, x, portable):
    """asinf / atanf / atan2f (FN_*; atan2f takes pairs {y, x}) of the host libm, or of the oracle's restatement."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    n = x.size // (2 if fn == FN_ATAN2F else 1)
    out = np.empty(n, np.float32)
    (lib.rtu_oracle_portable_libm if portable else lib.rtu_oracle_host_libm)(fn, x.ctypes.data, n, out.ctypes.data)
    return out


def check_portable(fn, first, count, seed=0, threads=8):
    """Restatement against the host libm on `count` inputs (see rtu_oracle.h): (mismatches, first failing input bits)."""
    fb = (ctypes.c_uint32 * 2)()
    n = lib.rtu_oracle_check_portable(fn, first, count, seed, threads, fb)
    return int(n), (int(fb[0]), int(fb[1]))


# the ray-level entry (rtu_oracle_rays): layouts of RtuRay / RtuRayHit (include/rtu_render.h), as the package's ray_dtype() / hit_dtype()
RAYS_CLOSEST, RAYS_OCCLUDED, RAYS_SHADE = 0, 1, 2
RAY_HIT, RAY_FRONT = 1, 2
RAY_DTYPE = np.dtype([("org", np.float32, 3), ("tmax", np.float32), ("dir", np.float32, 3), ("reserved", np.uint32)])
HIT_DTYPE = np.dtype([("t", np.float32), ("node", np.int32), ("flags", np.uint32), ("material", np.int32),
                      ("p", np.float32, 3), ("pad0", np.float32), ("N", np.float32, 3), ("pad1", np.float32)])
lib.rtu_oracle_rays.restype = ctypes.c_int
lib.rtu_oracle_rays.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                ctypes.POINTER(OracleStats), ctypes.c_int]


def _rays(scene, rays, mode, out, eye=None, stats=None, threads=1):
    rays = np.asarray(rays)
    if rays.dtype != RAY_DTYPE:
        if rays.dtype != np.float32 or rays.ndim != 2 or rays.shape[1] != 8:
            raise ValueError("rays: a structured array of the package's ray_dtype() or float32 [n, 8]")
    r = np.ascontiguousarray(rays).reshape(-1).view(RAY_DTYPE)
    assert len(out) == r.size
    e = np.ascontiguousarray(eye, np.float32) if eye is not None else None
    if e is not None and e.shape != (3,):
        raise ValueError("eye: three floats")
    rc = lib.rtu_oracle_rays(scene.desc_ptr, r.ctypes.data if r.size else None, r.size, e.ctypes.data if e is not None else None, mode,
                             out.ctypes.data if r.size else None, ctypes.byref(stats) if stats is not None else None, threads)
    if rc != 0:
        raise OracleError(rc)
    return out


def _n_rays(rays):
    rays = np.asarray(rays)
    return rays.size if rays.dtype == RAY_DTYPE else len(rays)


def trace_rays(scene, rays, threads=1):
    """Trace() along caller-supplied rays, HitInfo::Init's z replaced by tmax, dir as given, nothing filtered (valid rays only): a
    structured array [n] with the fields of RtuRayHit — what the device's rtu_trace_rays answers."""
    return _rays(scene, rays, RAYS_CLOSEST, np.zeros(_n_rays(rays), HIT_DTYPE), threads=threads)


def occluded_rays(scene, rays, threads=1):
    """ShadowTrace() along the rays, then `hit && hInfo.z > 0`: uint8 [n] — what rtu_occluded_rays answers."""
    return _rays(scene, rays, RAYS_OCCLUDED, np.zeros(_n_rays(rays), np.uint8), threads=threads)


def shade_rays(scene, rays, eye, threads=1, max_bounce=MAX_BOUNCE):
    """Trace() and Shade(..., max_bounce) along the rays with `eye` as camera.pos; a miss is the environment along dir with t = tmax:
    (float32 [n, 4] {r, g, b, t}, stats dict) — what rtu_shade_rays answers."""
    st = OracleStats()
    out = np.zeros((_n_rays(rays), 4), np.float32)
    with _bounces(max_bounce):
        _rays(scene, rays, RAYS_SHADE, out, eye=eye, stats=st, threads=threads)
    return out, st.as_dict()


# the keyed ray-level entry (rtu_oracle_rays_keyed): recipes S and P on caller-supplied rays and keys
KEYED_SAMPLED, KEYED_PATHS, KEYED_GATHER, KEYED_AMBIENT = 0, 1, 2, 3
INFO_HIT, INFO_FRONT, INFO_MATERIAL, INFO_GLOSSY = 1, 2, 4, 8
lib.rtu_oracle_rays_keyed.restype = ctypes.c_int
lib.rtu_oracle_rays_keyed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p,
                                      ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(OracleStats), ctypes.c_int]
lib.rtu_oracle_rays_keyed_info.restype = ctypes.c_int
lib.rtu_oracle_rays_keyed_info.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int]


def _keyed_args(rays, keys):
    rays = np.asarray(rays)
    if rays.dtype != RAY_DTYPE and (rays.dtype != np.float32 or rays.ndim != 2 or rays.shape[1] != 8):
        raise ValueError("rays: a structured array of the package's ray_dtype() or float32 [n, 8]")
    r = np.ascontiguousarray(rays).reshape(-1).view(RAY_DTYPE)
    k = np.ascontiguousarray(keys, np.uint32).reshape(-1)
    if k.size != r.size:
        raise ValueError("keys: one uint32 per ray")
    return r, k


def _keyed(scene, rays, keys, eye, mode, amb=None, threads=1, max_bounce=MAX_BOUNCE):
    r, k = _keyed_args(rays, keys)
    e = np.ascontiguousarray(eye, np.float32)
    if e.shape != (3,):
        raise ValueError("eye: three floats")
    a = None
    if mode == KEYED_AMBIENT:
        a = np.asarray(amb, np.float32).reshape(r.size, -1)
        if a.shape[1] == 3:
            a = np.concatenate([a, np.zeros((r.size, 1), np.float32)], axis=1)
        if a.shape[1] != 4:
            raise ValueError("amb: float32 [n, 4] or [n, 3]")
        a = np.ascontiguousarray(a)
    out = np.zeros((r.size, 4), np.float32)
    st = OracleStats()
    with _bounces(max_bounce):
        rc = lib.rtu_oracle_rays_keyed(scene.desc_ptr, r.ctypes.data if r.size else None, k.ctypes.data if r.size else None,
                                       a.ctypes.data if a is not None and r.size else None, r.size, e.ctypes.data, mode,
                                       out.ctypes.data if r.size else None, ctypes.byref(st), threads)
    if rc != 0:
        raise OracleError(rc)
    return out, st.as_dict()


def shade_rays_sampled(scene, rays, keys, eye, max_bounce=MAX_BOUNCE, threads=1):
    """Recipe S along the rays, keys[i] the key of ray i's root Shade() call: (float32 [n, 4] {r, g, b, t}, stats dict) — what
    rtu_shade_rays_sampled answers."""
    return _keyed(scene, rays, keys, eye, KEYED_SAMPLED, threads=threads, max_bounce=max_bounce)


def shade_rays_paths(scene, rays, keys, eye, max_bounce=MAX_BOUNCE, threads=1):
    """Recipe P along the rays (the 4-bounce gather behind every hit with a material) — what rtu_shade_rays_paths answers."""
    return _keyed(scene, rays, keys, eye, KEYED_PATHS, threads=threads, max_bounce=max_bounce)


def gather_rays(scene, rays, keys, eye, max_bounce=MAX_BOUNCE, threads=1):
    """{c.r, c.g, c.b, t}: the intensity of the AmbientLight MonteCarlo(hit, 4) appends for the ray's key — what rtu_gather_rays answers."""
    return _keyed(scene, rays, keys, eye, KEYED_GATHER, threads=threads, max_bounce=max_bounce)


def shade_rays_ambient(scene, rays, keys, amb, eye, max_bounce=MAX_BOUNCE, threads=1):
    """Recipe P with amb[i] (float32 [n, 4] {r, g, b, ignored} or [n, 3]) in place of the gathered light — what rtu_shade_rays_ambient
    answers."""
    return _keyed(scene, rays, keys, eye, KEYED_AMBIENT, amb=amb, threads=threads, max_bounce=max_bounce)


def keyed_info(scene, rays, keys, threads=1):
    """What keyed rays meet (rtu_oracle_rays_keyed_info): uint32 [n, 4] {INFO_* flags, gather rays of the chain that hit (0 .. 4),
    soft shadow rays of the root call, those of them that are occluded}."""
    r, k = _keyed_args(rays, keys)
    out = np.zeros((r.size, 4), np.uint32)
    rc = lib.rtu_oracle_rays_keyed_info(scene.desc_ptr, r.ctypes.data if r.size else None, k.ctypes.data if r.size else None, r.size,
                                        out.ctypes.data if r.size else None, threads)
    if rc != 0:
        raise OracleError(rc)
    return out
