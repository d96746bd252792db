#!/usr/bin/env python3
"""Extended soak of the fast variant against the counting variant on the random scenes of tests/test_gpu_fuzz.py (more seeds than
the test suite affords): both stage-2 forms, a ragged resolution, three shards, a batch of three turned cameras. Prints the seeds
that differ. usage: python tools/soak_fuzz.py FIRST_SEED LAST_SEED

SOAK_MODE=rays: the ray families of tests/test_fuzz_host.py (built from the device's own closest hits: no oracle) through the closest-hit,
occlusion and radiance entries, fast walk against reference walk. SOAK_MODE=update: the edit script and, where a scene has two meshes,
the chain of deformations of that file, an updated context against one that uploads each scene afresh, lists and structures against
the host builders."""
import os, random, sys, tempfile, pathlib
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import __graft_entry__ as g
import importlib.util
pkg = g.load_package()
spec = importlib.util.spec_from_file_location("fz", os.path.join(REPO, "tests", "test_gpu_fuzz.py"))
fz = importlib.util.module_from_spec(spec)
spec.loader.exec_module(fz)
d = fz.write_assets(pathlib.Path(tempfile.mkdtemp()))
first, last = int(sys.argv[1]), int(sys.argv[2])
only = [int(v) for v in os.environ.get("SOAK_SEEDS", "").split(",") if v]
dbg = int(os.environ.get("SOAK_DBG", "0"))
spp = int(os.environ.get("SOAK_SAMPLES", "0"))  # > 0: recipe S with that many samples per pixel (glossy bounces, soft shadows, lens); single frames and shards only
ctx = pkg.Context(0)
bad = []
W, H = 157, 99
def same(a, b, what, seed):
    eq = np.array_equal(a.view(np.uint32), b.view(np.uint32))
    if not eq:
        diff = np.argwhere((a.view(np.uint32) != b.view(np.uint32)).any(axis=-1))
        zdiff = int((a[..., 3].view(np.uint32) != b[..., 3].view(np.uint32)).sum())
        print("  seed %d: %s differs at %d pixels (%d in z), first %s: %s vs %s" % (seed, what, len(diff), zdiff, diff[0], a[tuple(diff[0])], b[tuple(diff[0])]), flush=True)
    return eq


def soak_rays(seed):
    """Fast walk against reference walk on R1-R4 of one seed: the bytes of all three entries."""
    scene = fh.w_scene(pkg, d, seed)
    ctx.upload(scene)
    eye, ok = fh.eye_of(scene), True
    for name, rays in fh.ray_families(pkg, None, scene, seed, trace=ctx.trace_rays):
        for what, call in (("closest hits", lambda ref: ctx.trace_rays(rays, reference_walk=ref)), ("occlusion", lambda ref: ctx.occluded(rays, reference_walk=ref)),
                           ("radiance", lambda ref: ctx.shade_rays(rays, eye, reference_walk=ref)[0])):
            fast, ref = np.ascontiguousarray(call(False)), np.ascontiguousarray(call(True))
            if not np.array_equal(fast.view(np.uint8), ref.view(np.uint8)):
                rows = np.argwhere((fast.view(np.uint8).reshape(rays.size, -1) != ref.view(np.uint8).reshape(rays.size, -1)).any(axis=1))
                print("  seed %d: %s, %s differ at %d rays, first %d" % (seed, name, what, len(rows), rows[0, 0]), flush=True)
                ok = False
    return ok


def soak_update(seed, other):
    """The edit script and the chain of deformations of one seed: `ctx` follows by updates, `other` uploads afresh."""
    import test_gpu_scene_update as su
    import test_mesh_update_host as mh
    scene = fh.w_scene(pkg, d, seed)
    ctx.upload(scene)
    ok = True

    def images_agree(now, what):
        fine = True
        for stats in (True, False):
            fr = pkg.frame_setup(now.desc.camera, W, H, collect_stats=stats)
            fine &= same(ctx.render(fr, stats=stats)[0], other.render(fr, stats=stats)[0], "%s, %s variant" % (what, "counting" if stats else "fast"), seed)
        try:
            su.assert_lists_equal(pkg, ctx, now, what)
        except AssertionError as e:
            print("  seed %d: %s" % (seed, e), flush=True)
            fine = False
        return fine
    for step, now in enumerate(fh.edit_script(pkg, scene, seed)):
        ctx.update(now)
        other.upload(now)
        ok &= images_agree(now, "edit step %d" % step)
    if scene.desc.n_meshes == 2:
        ctx.upload(scene)
        for now, ids, name in fh.mesh_script(pkg, scene):
            ctx.update_meshes(now, ids)
            other.upload(now)
            ok &= images_agree(now, name)
            try:
                for m in (0, 1):
                    mh.assert_same_structures(ctx.mesh_arrays(m), pkg.host_mesh(scene, m, now), "%s, mesh %d" % (name, m))
            except AssertionError as e:
                print("  seed %d: %s" % (seed, e), flush=True)
                ok = False
    return ok


mode = os.environ.get("SOAK_MODE", "")
if mode in ("rays", "update"):
    import test_fuzz_host as fh
    other = pkg.Context(0) if mode == "update" else None
    refused = []
    for seed in (only or range(first, last)):
        try:
            ok = soak_rays(seed) if mode == "rays" else soak_update(seed, other)
        except pkg.RtuError as e:  # a scene or a deformation beyond a device-path limit: refused, nothing to compare
            if e.code != pkg.RTU_ERR_UNSUPPORTED:
                raise
            refused.append(seed)
            continue
        if not ok:
            bad.append(seed)
            print("seed %d DIFFERS" % seed, flush=True)
        if seed % 25 == 0:
            print("... seed %d" % seed, flush=True)
    print("mode %s, seeds %d..%d: %d differ %s; %d refused as unsupported %s" % (mode, first, last - 1, len(bad), bad, len(refused), refused))
    if other is not None:
        other.close()
    ctx.close()
    sys.exit(0)
elif mode:
    sys.exit("SOAK_MODE must be rays or update")

for seed in (only or range(first, last)):
    rnd = random.Random(1000 + seed)
    xml = d / ("s%d.xml" % seed)
    xml.write_text(fz._make_stochastic(fz._scene_xml(rnd, d, seed % 3 == 2), rnd) if spp else fz._scene_xml(rnd, d, seed % 3 == 2))
    scene = pkg.Scene.from_xml(str(xml))
    ctx.upload(scene)
    if dbg:
        pkg.hip.rtu_debug_flags(ctx._h, dbg)
    cams = []
    for i in range(3):
        cam = type(scene.desc.camera).from_buffer_copy(scene.desc.camera)
        cam.pos[0] += 1.1 * i
        cam.fov += 7.0 * i
        cams.append(cam)
    kw = {"samples": spp} if spp else {}
    refs = [ctx.render(pkg.frame_setup(c, W, H, collect_stats=True, **kw), stats=True)[0] for c in (cams[:1] if spp else cams)]
    ok = True
    for thr in (10 ** 9, 1):
        fr = pkg.frame_setup(cams[0], W, H, **kw)
        fr.coop_threshold = thr
        ok &= same(ctx.render(fr)[0], refs[0], "single frame thr %d" % thr, seed)
        shards, frames = [], []
        for r in range(3):
            f = pkg.frame_setup(cams[0], W, H, shard_rank=r, shard_count=3, **kw)
            f.coop_threshold = thr
            shards.append(ctx.render(f)[0])
            frames.append(f)
        ok &= same(pkg.assemble(shards, frames, H), refs[0], "3 shards thr %d" % thr, seed)
        if spp:
            continue  # (frames in flight are recipe W)
        fb = [pkg.frame_setup(c, W, H) for c in cams]
        for f in fb:
            f.coop_threshold = thr
        dptr = pkg.hip.rtu_device_alloc(ctx._h, 3 * W * H * 16)
        for rep in range(3):  # (the later launches of the shape follow the habits the first taught the context: side mode, k_tail, grid hints)
            for attempt in range(17):  # the asynchronous entry's contract: render again until no level ran out of capacity (a level per round at worst)
                ctx.render_frames_device(fb, dptr, None)
                try:
                    ctx.frame_status()
                    break
                except pkg.RtuError as e:
                    if e.code != pkg.RTU_ERR_CAPACITY or attempt == 16:
                        raise
            out = np.empty((3, H, W, 4), np.float32)
            pkg.hip.rtu_copy_to_host(ctx._h, out.ctypes.data, dptr, out.nbytes)
            for i in range(3):
                ok &= same(out[i], refs[i], "batch frame %d thr %d launch %d" % (i, thr, rep), seed)
        pkg.hip.rtu_device_free(ctx._h, dptr)
    if not ok:
        bad.append(seed)
        print("seed %d DIFFERS" % seed, flush=True)
    if seed % 25 == 0:
        print("... seed %d" % seed, flush=True)
print("seeds %d..%d: %d differ %s" % (first, last - 1, len(bad), bad))
ctx.close()
