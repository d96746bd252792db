"""GPU: temporal sessions over long, mixed lifetimes against a hand model (include/rtu_render.h "Temporal accumulation", "... across
scene updates", "Variance-guided filtering", "Steered sampling", "Temporal gradients", "Sparse sessions"). The pieces are tested
elsewhere — device forms against host forms, host forms against restatements; a session's frames against the hand form over a few
frames of one kind of call. Here one script of 24 frames mixes every kind of call in one session of every kind, at 67 x 35 (ragged
for the 3 x 3 strata and for blocks of 2, 3 and 4) with max_history 3, and a model that holds nothing but the session's documented
state (HandSession) says what every frame must be, bit for bit, out of the existing hand_frame helpers.

What the existing session tests do not run, and the step of make_script() that does:
    gap                                                                                        step
     1  plain and moved frames mixed in one session, bit for bit                               1-2, 4-6, 8-10
     2  rtu_update_meshes (RTU_MOTION_RESET entries) in a variance, steered, gradient or
        sparse session                                                                         9
     3  a moved frame after rtu_upload_scene of a scene with another node count: the table
        buffers grow in the middle of a session, a later call is checked against the new count 10
     4  two updates between two frames, the table taken from the two scenes that were rendered 5
     5  samples, max_bounce, gather_bounces that differ from the previous frame's              7
     6  more frames than max_history inside a session                                          1 (and every later one)
     7  rtu_temporal_reset in the middle of a run, then a moved frame as frame 0 with a NULL
        table                                                                                  8
     8  the device forms on a caller's stream for steered, gradient and sparse sessions        every odd frame
     9  other work on the same context between two frames                                      between all frames
    10  a refused call in the middle leaves every kind as it was                               3, 4 (with an update pending), 10

After step 9 a pixel of the deformed mesh has n == 1 in a plain, variance or gradient session; min(1 + its extra rays, max_history)
in a steered one, which folds them into the fresh pixel; and in a sparse session 1 if it is its block's owner and 0 (no colour, a
hole) if not. Step 10 uploads p9_s3_160x120 (13 nodes against 9; p11_p2_120x68 has 9 as well and would grow no table). Step 4 takes
history_cap 2, which with max_history 3 changes no dense frame (min(n, 2) + 1 == min(n + 1, 3)); step 5 takes cap 1, which binds.

What the script found when it was written: a call refused late left its mark. A plain frame with max_bounce 6 after an update
(step 4) was refused by the shading entry AFTER the session had taken the new scene generation and dropped its history, so the moved
frame that followed had none (a camera position that is not finite did the same); a steered frame with samples * (1 + max_extra) > 65536 (step 3) was refused by the extra-ray entry
after the histories were swapped and k had advanced. temporal_frame() now commits its state in one place, behind the last entry
that can refuse, and refuses the steered case up front.

The other work is, in rotation, a render, a ray query of the camera rays and a step of a progressive session. The render is a
two-sample recipe S frame of another size: the scene has glossy and soft effects, so a recipe W frame is refused before anything
is launched and would be no work at all.

The last test runs the K = 40 frame chains at rest of tests/test_temporal_mean_host.py through the device forms on caller-owned
histories and applies that module's float64 checks: a history at rest is the mean of its samples, said of the kernels directly."""
import ctypes

import numpy as np
import pytest

import test_gpu_gradient as G
import test_gpu_sparse as P
import test_gpu_steer as S
import test_gpu_temporal as T
import test_gpu_temporal_motion as M
import test_gpu_variance as V
import test_temporal_mean_host as R
from test_gpu_ray_query import bits
from test_gpu_temporal import dev, orbit_frames
from test_gpu_temporal_motion import MESH_NODE, animated
from test_gpu_variance import fresh
from test_mesh_update_host import deformed_scene
from test_sparse_host import np_owners
from test_temporal_motion_host import RESET, STATIC, table

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 67, 35
MAX_HISTORY = 3
KINDS = {"plain": {}, "denoise": {"denoise": True}, "variance": {"variance": True}, "steered": {"variance": True, "steer": True},
         "gradient-variance": {"variance": True, "gradient": True}, "gradient-steered": {"variance": True, "steer": True, "gradient": True},
         "sparse2": {"variance": True, "block": 2}, "sparse3": {"variance": True, "block": 3}}


def descs(pkg, kind):
    o = KINDS[kind]
    return {"desc": pkg.temporal_desc(W, H, denoise=o.get("denoise", False), max_history=MAX_HISTORY),
            "variance": pkg.variance_desc(W, H) if o.get("variance") else None,
            "steer": pkg.steer_desc(budget=W * H // 2, max_extra=3) if o.get("steer") else None,      # about half a ray per pixel
            "gradient": pkg.gradient_desc(radius=1, kappa=0.5) if o.get("gradient") else None,         # a low floor: lambda rises under motion
            "sparse": pkg.sparse_desc(block=o["block"]) if o.get("block") else None}


def open_session(pkg, ctx, kind):
    d = descs(pkg, kind)
    return ctx.temporal(d["desc"], variance=d["variance"], steer=d["steer"], gradient=d["gradient"], sparse=d["sparse"])


# ---- the model ------------------------------------------------------------------------------------------------------------------------
class HandSession:
    """What a session is, by include/rtu_render.h, as state and nothing else: the frame counter k, the previous frame's desc and
    history (a gradient session: and the luminance plane of its sample), and the scene generation the session has seen. Every frame
    is made by the existing hand_frame helpers from public entries on the same context; there is no arithmetic here. The rules:
      - k = 0 and no history at begin and after reset ("Temporal accumulation": "counted from 0 since rtu_temporal_begin or the
        last rtu_temporal_reset").
      - A plain frame that finds another scene generation starts over: k = 0, no history, a gradient session takes no lambda
        ("Temporal accumulation": "the next frame starts over with no history and k = 0"; "Temporal gradients", THE SESSION).
      - A moved frame adopts the generation and keeps both ("... across scene updates", THE SESSION (a)). Without a previous frame
        its table is not used ("On frame 0 the table is not used").
      - A plain frame with history is a moved frame with an all-STATIC table and history_cap 0 ("... across scene updates": "an
        all-STATIC table with history_cap 0 gives the bits of rtu_temporal_accumulate"; "Variance-guided filtering", THE SESSION).
      - The samples, owners and dithers of frame k are taken with the S of the frame given in that call ("Temporal accumulation",
        A session that drives it: "may differ from call to call").
      - A refused call changes nothing: the model is not told of it."""

    def __init__(self, pkg, ctx, kind):
        self.pkg, self.ctx, self.kind, self.d = pkg, ctx, kind, descs(pkg, kind)
        self.gen = None
        self.reset()

    def reset(self):
        self.k, self.prev, self.hist, self.lum = 0, None, None, None

    def frame(self, frame, moved, gen, n_nodes):
        """moved: None for a plain frame, (table or None, history_cap) for a moved one; gen: the context's scene generation."""
        pkg, ctx, d, o = self.pkg, self.ctx, self.d, KINDS[self.kind]
        if gen != self.gen:
            if moved is None:
                self.reset()
            self.gen = gen
        res = {"started_over": self.hist is None, "k": self.k, "lam": None, "holes": None, "counts": None, "total": None}
        motion, cap = (table("static", n_nodes), 0) if moved is None or self.hist is None else moved
        if "block" in o:
            res["image"], hist, res["holes"] = P.hand_frame(pkg, ctx, frame, self.k, self.prev, self.hist, d["desc"], d["variance"], o["block"], motion, cap)
        elif "gradient" in o:
            st = {}
            res["image"], (hist, self.lum), res["lam"] = G.hand_frame(pkg, ctx, frame, self.k, self.prev, None if self.hist is None else (self.hist, self.lum),
                                                                      d["desc"], d["variance"], d["steer"], d["gradient"], motion, cap, steer_out=st)
            res["counts"], res["total"] = st.get("counts"), st.get("total")
        elif "steer" in o:
            res["image"], hist, _, res["counts"], res["total"] = S.hand_frame(pkg, ctx, frame, self.k, self.prev, self.hist, d["desc"], d["variance"], d["steer"], motion, cap)
        elif "variance" in o:
            res["image"], hist, _, _ = V.hand_frame(pkg, ctx, frame, self.k, self.prev, self.hist, d["desc"], d["variance"], motion, cap)
        elif self.hist is None:
            res["image"], hist, _ = T.hand_frame(pkg, ctx, frame, self.k, None, None, d["desc"], o.get("denoise", False))
        else:
            res["image"], hist, _ = M.hand_frame_moved(pkg, ctx, frame, self.k, self.prev, self.hist, d["desc"], o.get("denoise", False), motion, cap)
        self.k, self.prev, self.hist = self.k + 1, frame, hist
        res["n"] = hist[0][..., 3]
        return res


# ---- the script -----------------------------------------------------------------------------------------------------------------------
def make_script(pkg, golden, last_step=10):
    """The steps as a list of operations: ("frame", step, frame, moved, at_rest), ("refuse", step, what, frame, moved, the key of
    KINDS it is refused for or None for all), ("update" | "update_meshes" | "upload", scene), ("reset",). moved: None for a plain call,
    (table or None, history_cap) for a moved one. at_rest: the camera, the scene and the frame's recipe are those of the
    frame before, which was no start-over: a gradient session's lambda is exactly 0."""
    base = golden("p10_s4_160x120").scene(pkg)
    room = golden("p9_s3_160x120").scene(pkg)  # 13 nodes against 9 (p11_p2_120x68 has 9 too: its upload would grow nothing)
    n_old, n_new = base.desc.n_nodes, room.desc.n_nodes
    assert n_old != n_new, "step 10 needs a scene with another node count"
    A = animated(pkg, base, 4, 20.0, 0.2)  # the mesh node and a sphere moved a step further in each; A[2] also turns the camera
    kw = {"samples": 3}
    rest = pkg.frame_setup(base.desc.camera, W, H, **kw)
    orbit = orbit_frames(pkg, base, W, H, 4, 20.0, 0.5, **kw)[1:]
    still = table("static", n_old)
    ops = []
    fr = lambda step, frame, moved=None, at_rest=False: ops.append(("frame", step, frame, moved, at_rest))
    ops.append(("upload", A[0]))
    for i in range(4):                                                    # 1. at rest: the one-tap path; n reaches 3 and stays
        fr(1, rest, at_rest=i > 0)
    for f in orbit:                                                       # 2. reprojection
        fr(2, f)
    ops.append(("refuse", 3, "a frame of another size", pkg.frame_setup(base.desc.camera, W + 1, H, **kw), None, None))   # 3. refused calls
    ops.append(("refuse", 3, "n_nodes - 1 entries", rest, (still[:-1], 2), None))
    ops.append(("refuse", 3, "history_cap -1", rest, (still, -1), None))
    ops.append(("refuse", 3, "samples * (1 + max_extra) > 65536", pkg.frame_setup(base.desc.camera, W, H, samples=16385), None, "steer"))
    ops.append(("update", A[1]))                                          # 4. nodes moved, the table of rtu_scene_motion, cap 2
    ops.append(("refuse", 4, "max_bounce 6, a plain frame with an update pending", pkg.frame_setup(base.desc.camera, W, H, max_bounce=6, **kw), None, None))
    blind = pkg.frame_setup(base.desc.camera, W, H, **kw)                 # (refused by the shading entry, deep inside the frame)
    blind.cam_pos[0] = float("nan")
    ops.append(("refuse", 4, "a camera position that is not finite, a plain frame with an update pending", blind, None, None))
    fr(4, pkg.frame_setup(A[1].desc.camera, W, H, **kw), (pkg.scene_motion(A[0], A[1]), 2))
    ops.append(("update", A[2]))                                          # 5. two updates, the table of first against last rendered scene
    ops.append(("update", A[3]))
    fr(5, pkg.frame_setup(A[3].desc.camera, W, H, **kw), (pkg.scene_motion(A[1], A[3]), 1))  # (cap 1: below max_history - 1, so it binds)
    ops.append(("update", A[0]))                                          # 6. an update, then a plain frame: it starts over
    fr(6, rest)
    if last_step == 6:
        return ops, n_old, n_new
    for i in range(2):                                                    # 7. S 3 -> 5; max_bounce; recipe P; and back
        fr(7, pkg.frame_setup(base.desc.camera, W, H, samples=5), at_rest=i > 0)
    fr(7, pkg.frame_setup(base.desc.camera, W, H, samples=3, max_bounce=2))
    for i in range(2):
        fr(7, pkg.frame_setup(base.desc.camera, W, H, samples=3, gather_bounces=4), at_rest=i > 0)
    for i in range(4):
        fr(7, rest, at_rest=i > 0)
    ops.append(("reset",))                                                # 8. reset; a moved frame as frame 0 with a NULL table; a moved frame
    fr(8, rest, (None, 2))
    ops.append(("update", A[1]))
    fr(8, pkg.frame_setup(A[1].desc.camera, W, H, **kw), (pkg.scene_motion(A[0], A[1]), 2))
    wobble = deformed_scene(pkg, A[1], 0, ("wobble", 1))                  # 9. a deformed mesh: RTU_MOTION_RESET
    motion = pkg.scene_motion(A[1], wobble, reset_meshes=[0])
    assert [i for i in range(n_old) if motion["flags"][i] & RESET] == [MESH_NODE] and (motion["flags"] & STATIC).all()
    ops.append(("update_meshes", wobble))
    fr(9, pkg.frame_setup(wobble.desc.camera, W, H, **kw), (motion, 0))
    there = pkg.frame_setup(room.desc.camera, W, H, **kw)                 # 10. a scene with another node count
    ops.append(("upload", room))
    fr(10, there, (table("static", n_new), 0))
    ops.append(("refuse", 10, "a table of the old node count", there, (still, 0), None))
    fr(10, there)
    return ops, n_old, n_new


class Player:
    """Plays a script on one context for one or more sessions, frame by frame in turn: every other successful frame of a session through
    the device form on the test's stream (ONE STREAM PER CONTEXT: synchronised before the next call), the rest through the host form;
    other work on the context between the frames."""

    def __init__(self, pkg, ctx, other_work=True):
        import torch
        self.pkg, self.ctx, self.gen, self.n_nodes = pkg, ctx, 0, 0
        self.stream = torch.cuda.Stream(device=0)
        self.d_out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        self.d_counts = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
        self.other_work, self.turn, self.prog = other_work, 0, None
        self.scene = self.step9_masks = None

    def world(self, op):
        if self.prog is not None:
            self.prog.close()
            self.prog = None
        if op[0] == "upload":
            self.ctx.upload(op[1])
        elif op[0] == "update":
            self.ctx.update(op[1])
        else:
            self.ctx.update_meshes(op[1], [0])
        self.scene, self.gen, self.n_nodes = op[1], self.gen + 1, op[1].desc.n_nodes

    def other(self):
        """Between two frames, in rotation: a render, a ray query, a step of a progressive session."""
        if not self.other_work:
            return
        pkg, cam = self.pkg, self.scene.desc.camera
        if self.turn % 3 == 0:
            self.ctx.render(pkg.frame_setup(cam, 48, 27, samples=2))
        elif self.turn % 3 == 1:
            self.ctx.trace_rays(pkg.camera_rays(pkg.frame_setup(cam, 40, 30)))
        else:
            if self.prog is None:
                self.prog = self.ctx.progressive(pkg.frame_setup(cam, 32, 24, samples=64))
            self.prog.advance(1)
        self.turn += 1

    def call(self, s, frame, moved, device):
        """One session call -> (rc, image or None): by the C entries, so that a NULL table and a refusal need no other path."""
        pkg, hip = self.pkg, self.pkg.hip
        f = ctypes.byref(frame)
        out = np.empty((H, W, 4), F)
        if moved is not None:
            motion, cap = moved
            m = None if motion is None else np.ascontiguousarray(motion)
            args = (m.ctypes.data if m is not None else None, self.n_nodes if m is None else len(m), int(cap))
        if device:
            assert hip.rtu_context_sync(self.ctx._h) == pkg.RTU_OK
            if moved is None:
                rc = hip.rtu_temporal_frame_device(s._h, f, self.d_out.data_ptr(), self.stream.cuda_stream)
            else:
                rc = hip.rtu_temporal_frame_moved_device(s._h, f, *args, self.d_out.data_ptr(), self.stream.cuda_stream)
            self.stream.synchronize()
            if rc == pkg.RTU_OK:
                out = self.d_out.cpu().numpy()
        elif moved is None:
            rc = hip.rtu_temporal_frame(s._h, f, out.ctypes.data)
        else:
            rc = hip.rtu_temporal_frame_moved(s._h, f, *args, out.ctypes.data)
        return rc, (out if rc == pkg.RTU_OK else None)

    def observe(self, s, kind, device=False):
        """Everything a session shows of itself besides the image."""
        o = KINDS[kind]
        got = {"n": s.history()}
        if "gradient" in o:
            got["lam"] = s.lambda_image()
        if "block" in o:
            got["holes"] = s.holes()
        if "steer" in o:
            got["total"] = s.steer_total()
            if device:  # rtu_temporal_extra_counts_device on the caller's stream
                s.extra_counts_device(self.d_counts.data_ptr(), self.stream.cuda_stream)
                self.stream.synchronize()
                got["counts"] = self.d_counts.cpu().numpy().view(np.uint32)
            else:
                got["counts"] = s.extra_counts()
        return got

    def close(self):
        if self.prog is not None:
            self.prog.close()


def same(a, b):
    if isinstance(a, np.ndarray):
        return np.array_equal(bits(a) if a.dtype == F else a, bits(b) if b.dtype == F else b)
    return a == b


def differing(what, got, want):
    if isinstance(got, np.ndarray):
        g, w = (bits(got), bits(want)) if got.dtype == F else (got, want)
        diff = g.reshape(w.shape) != w
        return "%s: %d words differ, first at %s" % (what, diff.sum(), np.argwhere(diff)[0])
    return "%s: %s, the model says %s" % (what, got, want)


# ---- one script per kind against the model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_long_mixed_session_equals_the_hand_model(pkg, golden, kind):
    o = KINDS[kind]
    ops, n_old, n_new = make_script(pkg, golden)
    ctx = pkg.Context(0)
    play = Player(pkg, ctx)
    s = open_session(pkg, ctx, kind)
    model = HandSession(pkg, ctx, kind)
    seen, recs, tables = set(), [], set()
    try:
        for op in ops:
            if op[0] in ("upload", "update", "update_meshes"):
                play.world(op)
            elif op[0] == "reset":
                s.reset()
                model.reset()
                assert not s.history().any()
            elif op[0] == "refuse":
                _, step, what, frame, moved, only = op
                if only is not None and only not in o:
                    continue
                before = play.observe(s, kind)
                rc, _ = play.call(s, frame, moved, device=len(recs) % 2 == 1)
                assert rc == pkg.RTU_ERR_ARG, "step %d, %s: rc %d" % (step, what, rc)
                after = play.observe(s, kind)
                for key in before:
                    assert same(after[key], before[key]), "step %d, refused call (%s) changed %s" % (step, what, key)
            else:
                _, step, frame, moved, at_rest = op
                idx = len(recs)
                where = "%s step %d frame %d (%s, %s form)" % (kind, step, idx, "moved" if moved else "plain", "device" if idx % 2 else "host")
                play.other()
                had_history = model.hist is not None and not (moved is None and model.gen != play.gen)
                a0 = pkg.hip.rtu_debug_device_allocations()
                rc, got = play.call(s, frame, moved, device=idx % 2 == 1)
                a1 = pkg.hip.rtu_debug_device_allocations()
                assert rc == pkg.RTU_OK, "%s: rc %d" % (where, rc)
                key = (moved is not None, frame.gather_bounces != 0, play.n_nodes)
                assert key not in seen or a1 == a0, "%s allocated, after a frame of the same call kind, recipe and node count" % where
                seen.add(key)
                shown = play.observe(s, kind, device=idx % 2 == 1)
                want = model.frame(frame, moved, play.gen, play.n_nodes)
                assert same(got, want["image"]), differing(where + " image", got, want["image"])
                for k2, v in shown.items():
                    assert same(v, want[k2]), differing("%s %s" % (where, k2), v, want[k2])
                if moved is not None and had_history:
                    tables.add(play.n_nodes)
                if step == 9:  # the guides of the deformed scene, while the context holds it
                    hits = ctx.frame_features(frame)[0]
                    valid = ((hits["flags"] & 1) != 0).reshape(H, W)
                    play.step9_masks = (valid & (hits["node"].reshape(H, W) == MESH_NODE), valid, np.isfinite(got[..., :3]).all(-1))
                recs.append(dict(want, step=step, at_rest=at_rest, moved=moved is not None, frame=frame))
        # ---- the script reached what it is there for ----
        n = [r["n"] for r in recs]
        assert len(recs) == 24 and max(r["k"] for r in recs) > MAX_HISTORY
        assert any(((n[i] == MAX_HISTORY) & (n[i + 1] == MAX_HISTORY)).any() for i in range(len(n) - 1)), "no pixel stayed at max_history"
        assert max(float(x.max()) for x in n) == MAX_HISTORY
        overs = [i for i, r in enumerate(recs) if r["started_over"] and i > 0]
        assert len(overs) >= 2, "start-overs at %s" % overs
        assert tables == {n_old, n_new}, "moved frames with a history used tables of %s nodes" % sorted(tables)
        i9 = [i for i, r in enumerate(recs) if r["step"] == 9][0]
        on_mesh, valid, fin = play.step9_masks
        k9 = recs[i9]["k"]
        # what "n == 1" is per kind: a steered session folds its extra samples into the fresh pixel, n = min(1 + count, max_history);
        # in a sparse session only a block's owner takes a sample, a RESET pixel that is none has no colour at all, n = 0
        want_n = np.ones((H, W), F)
        if recs[i9]["counts"] is not None:
            want_n = np.minimum(1 + recs[i9]["counts"].reshape(H, W), MAX_HISTORY).astype(F)
        if "block" in o:
            x, y, _, _ = np_owners(W, H, o["block"], k9)
            own = np.zeros((H, W), bool)
            own[y, x] = True
            want_n = np.where(own, want_n, F(0))
        assert (on_mesh & fin).sum() >= 50, "%d pixels show the deformed mesh with a finite colour" % (on_mesh & fin).sum()
        assert np.array_equal(n[i9][on_mesh & fin], want_n[on_mesh & fin]), "a deformed surface kept its history"
        assert (n[i9][valid & ~on_mesh] > 1).any(), "the rest lost its history"
        if "gradient" in o:
            assert any(r["lam"].any() for r in recs if r["step"] in (4, 5)), "lambda is 0 after the nodes moved"
            rest = [r for r in recs if r["at_rest"]]
            assert len(rest) >= 8 and not any(bits(r["lam"]).any() for r in rest), "lambda != 0.0 at rest"
            assert not any(r["lam"].any() for r in recs if r["started_over"]), "a frame that started over took a gradient"
        if "block" in o:
            b2 = o["block"] ** 2
            i6 = [i for i, r in enumerate(recs) if r["step"] == 6][0]
            assert recs[i6]["started_over"] and recs[i6]["k"] == 0 and recs[i6 + b2]["k"] == b2
            assert recs[i6]["holes"] > 0 and recs[i6 + b2]["holes"] < recs[i6]["holes"], "holes %s" % [r["holes"] for r in recs]
        if "steer" in o:
            spent = [r["total"] for r in recs]
            assert sum(t > 0 for t in spent) * 2 >= len(spent), "extra rays per frame: %s" % spent
        print("%s: n max %g, start-overs at %s, mesh pixels %d, holes %s, extra rays %s" % (
            kind, max(float(x.max()) for x in n), overs, on_mesh.sum(), [r["holes"] for r in recs] if "block" in o else "-",
            [r["total"] for r in recs] if "steer" in o else "-"))
    finally:
        play.close()
        s.close()
        ctx.close()


# ---- two sessions on one context --------------------------------------------------------------------------------------------------------
def record(pkg, golden, kinds, ops):
    """The script for the sessions `kinds` on one fresh context, advanced alternately: per kind the list of (image, what it shows)."""
    ctx = pkg.Context(0)
    play = Player(pkg, ctx)
    sessions = [open_session(pkg, ctx, kind) for kind in kinds]
    out = {kind: [] for kind in kinds}
    try:
        for op in ops:
            if op[0] in ("upload", "update", "update_meshes"):
                play.world(op)
            elif op[0] == "refuse":
                _, step, what, frame, moved, only = op
                for s, kind in zip(sessions, kinds):
                    if only is None or only in KINDS[kind]:
                        assert play.call(s, frame, moved, device=False)[0] == pkg.RTU_ERR_ARG, "%s step %d, %s" % (kind, step, what)
            else:
                _, step, frame, moved, _ = op
                play.other()
                for s, kind in zip(sessions, kinds):
                    device = len(out[kind]) % 2 == 1
                    rc, got = play.call(s, frame, moved, device)
                    assert rc == pkg.RTU_OK, "%s step %d: rc %d" % (kind, step, rc)
                    out[kind].append((step, got, play.observe(s, kind, device)))
    finally:
        play.close()
        for s in sessions:
            s.close()
        ctx.close()
    return out


def test_two_sessions_on_one_context_are_each_the_session_alone(pkg, golden):
    """A gradient-on-steered and a sparse session advanced alternately through steps 1-6 on one context: the shared frame records,
    the steered session's read-back and the sparse session's event leave each the session it is alone on a fresh context."""
    kinds = ["gradient-steered", "sparse2"]
    ops = make_script(pkg, golden, last_step=6)[0]
    both = record(pkg, golden, kinds, ops)
    for kind in kinds:
        alone = record(pkg, golden, [kind], ops)[kind]
        assert len(alone) == len(both[kind]) == 10
        for i, ((step, img, shown), (_, want_img, want)) in enumerate(zip(both[kind], alone)):
            where = "%s step %d frame %d" % (kind, step, i)
            assert same(img, want_img), differing(where + " image", img, want_img)
            for key, v in shown.items():
                assert same(v, want[key]), differing("%s %s" % (where, key), v, want[key])


# ---- a history at rest is the mean of its samples: the device forms ------------------------------------------------------------------------
def test_device_histories_at_rest_are_the_means_of_their_samples(pkg):
    """The chains of tests/test_temporal_mean_host.py at 67 x 35 through rtu_temporal_accumulate_moments_device, _gradient_device and
    _sparse_device on caller-owned histories, on a caller's stream; that module's float64 checks on what comes back."""
    import torch
    inp = R.rest_inputs(pkg, W, H)
    cam, n = inp["cam"], W * H
    ctx = pkg.Context(0)  # no scene: the entries need none
    stream = torch.cuda.Stream(device=0)
    d_hits, d_alb, d_motion = dev(inp["hits"]), dev(inp["albedo"]), dev(inp["still"])
    desc = pkg.temporal_desc(W, H, max_history=R.K)
    back = lambda d, shape: d.cpu().numpy().view(F).reshape(shape).copy()
    prev = [None]

    def dense(call):
        def form(k, f, h):
            d_in, d_hist, d_out = dev(f), fresh(64 * n), fresh(16 * n)
            call(desc, cam if k else None, cam, d_in.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), prev[0].data_ptr() if k else None, d_hist.data_ptr(),
                 d_out.data_ptr(), d_motion.data_ptr(), 1, 0)
            stream.synchronize()
            prev[0] = d_hist
            return back(d_out, (H, W, 4)), back(d_hist, (4, H, W, 4))
        return form
    try:
        res = R.dense_ratios(inp, R.dense_chain(inp, dense(lambda *a: ctx.temporal_accumulate_moments_device(*a, stream=stream.cuda_stream))))
        R.report("moments, device form", inp, res)
        assert R.within(res), res
        d_lam = dev(np.full(((H + 2) // 3) * ((W + 2) // 3), 0.25, F))
        outs = R.dense_chain(inp, dense(lambda *a: ctx.temporal_accumulate_gradient_device(*a, d_lam.data_ptr(), stream=stream.cuda_stream)))
        res = R.dense_ratios(inp, outs, precap=3)
        R.report("gradient, device form", inp, res)
        assert R.within(res), res
        assert R.dense_ratios(inp, outs, precap=3, off=1)["E"] > 1, "the weight 1 / (n + 2) passed the same check"
        for B in R.BLOCKS:
            sd = pkg.sparse_desc(W, H, block=B)

            def sparse(k, rgbt, owner, h):
                d_rgbt, d_owner, d_hist, d_out, d_hole = dev(rgbt), dev(owner), fresh(64 * n), fresh(16 * n), fresh(n)
                ctx.temporal_accumulate_sparse_device(desc, sd, cam if k else None, cam, d_rgbt.data_ptr(), d_owner.data_ptr(), d_hits.data_ptr(),
                                                      d_alb.data_ptr(), prev[0].data_ptr() if k else None, d_hist.data_ptr(), d_out.data_ptr(),
                                                      d_hole.data_ptr(), d_motion.data_ptr(), 1, 0, stream.cuda_stream)
                stream.synchronize()
                prev[0] = d_hist
                return back(d_out, (H, W, 4)), back(d_hist, (4, H, W, 4)), d_hole.cpu().numpy().reshape(H, W)
            outs = R.sparse_chain(inp, B, sparse)
            res = R.sparse_ratios(inp, B, outs)
            R.report("sparse block %d, device form" % B, inp, res)
            assert R.sparse_within(res), res
            assert R.sparse_ratios(inp, B, outs, non_owners_blend=True)["E"] > 1, "a reference whose non-owners blend passed the same check"
    finally:
        ctx.close()
