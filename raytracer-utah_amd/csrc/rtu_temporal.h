// rtu_temporal.h — the arithmetic of the temporal accumulator (include/rtu_render.h "Temporal accumulation", "... across scene
// updates" and the moments of "Variance-guided filtering"), host + device, and the launch interface of its kernels (rtu_temporal.hip),
// called by rtu_capi_temporal.hip. The three forms — rtu_temporal_accumulate, _motion and _moments, each with its _device form — are the
// instantiations of one function, tp_pixel<MOVING, MOMENTS>; rtu_temporal_accumulate_gradient ("Temporal gradients") is a fourth,
// tp_pixel<true, true, true>, and rtu_temporal_accumulate_sparse ("Sparse sessions") a fifth, tp_pixel<true, true, false, true>.
// rtu_temporal_accumulate_sensor and _sensor_moments ("Temporal accumulation for sensors") are tp_pixel<false, MOMENTS> with another
// projection, TpSensorProj<MODEL> in place of the pinhole; that projection has the one transcendental function, sensor_acos.
//
// A pixel's first-hit point is projected into the previous camera, the history is fetched there with four bilinear taps, each tested
// for being the same surface, and the new sample is blended in. No transcendental function: the translation units that include this
// header are compiled with -ffp-contract=off and IEEE divides and square roots, every operation below rounds once, so the host forms
// and the kernels give the same bits.
//
// A HISTORY is three planes of one float4 per pixel:  E = {e.rgb, n}   P = {p.xyz, t}   N = {N.xyz, node as bits}
// A MOMENTS HISTORY has a fourth:  M = {m1, m2, 0, 0}, the running first and second moment of the luminance of the demodulated sample.
#ifndef RTU_TEMPORAL_H_INCLUDED
#define RTU_TEMPORAL_H_INCLUDED

#include "rtu_denoise.h"
#include "rtu_sensor.h"

#include <type_traits>

#define TP_LOOKUP_NONE      0  // no previous history
#define TP_LOOKUP_STATIC    1  // the cameras are equal bit for bit: the pixel itself with weight 1
#define TP_LOOKUP_REPROJECT 2
#define TP_STRATUM          3  // the strata of "Temporal gradients" are TP_STRATUM x TP_STRATUM pixels

// what a pixel needs of the desc and of the PREVIOUS camera; made once per call by tp_setup on the host, for both forms
struct TpParams {
    int32_t width, height, lookup;
    float   max_history, sigma_plane, normal_min;
    float   pos[3], origin[3], u[3], v[3];
    float   nrm[3];      // u x v
    float   num;         // dot(origin - pos, nrm)
    float   uu, vv;      // dot(u, u), dot(v, v)
};

inline bool tp_same_camera(const RtuFrameDesc& a, const RtuFrameDesc& b) {
    union { float f; uint32_t u; } x, y;
    if (a.width != b.width || a.height != b.height) return false;
    for (int k = 0; k < 3; k++) {
        const float fa[4] = {a.cam_pos[k], a.origin[k], a.u[k], a.v[k]}, fb[4] = {b.cam_pos[k], b.origin[k], b.u[k], b.v[k]};
        for (int j = 0; j < 4; j++) {
            x.f = fa[j]; y.f = fb[j];
            if (x.u != y.u) return false;
        }
    }
    return true;
}

inline TpParams tp_setup(const RtuTemporalDesc& d, const RtuFrameDesc& prev, const RtuFrameDesc& cur, bool has_prev) {
    TpParams p{};
    p.width = d.width;
    p.height = d.height;
    p.lookup = !has_prev ? TP_LOOKUP_NONE : (tp_same_camera(prev, cur) ? TP_LOOKUP_STATIC : TP_LOOKUP_REPROJECT);
    p.max_history = (float)d.max_history;
    p.sigma_plane = d.sigma_plane;
    p.normal_min = d.normal_min;
    const f3 pos = ld3(prev.cam_pos), origin = ld3(prev.origin), u = ld3(prev.u), v = ld3(prev.v);
    const f3 nrm = cross3(u, v);
    for (int k = 0; k < 3; k++) { p.pos[k] = prev.cam_pos[k]; p.origin[k] = prev.origin[k]; p.u[k] = prev.u[k]; p.v[k] = prev.v[k]; }
    p.nrm[0] = nrm.x; p.nrm[1] = nrm.y; p.nrm[2] = nrm.z;
    p.num = dot3(origin - pos, nrm);
    p.uu = dot3(u, u);
    p.vv = dot3(v, v);
    return p;
}

// float4 i of a caller's floats, which need not be 16-byte aligned (the host forms)
inline float4 f4(const float* p, size_t i) { return make_float4(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]); }
inline void st4(float* p, size_t i, const float4& v) { p[4 * i] = v.x; p[4 * i + 1] = v.y; p[4 * i + 2] = v.z; p[4 * i + 3] = v.w; }

RTU_HD bool tp_finite(float x) { return (x - x) == 0.0f; }  // false for an infinity and for a NaN

// ---- moving nodes (include/rtu_render.h "Temporal accumulation across scene updates") ------------------------------------------------
// What the motion form needs beyond TpParams; made once per call by tp_motion_setup. P.lookup is TP_LOOKUP_NONE or TP_LOOKUP_REPROJECT
// here: whether a pixel takes the one tap is decided per pixel (same_cam and its node's RTU_MOTION_STATIC).
struct TpMotionParams {
    TpParams P;
    int32_t  same_cam;  // the two cameras are equal bit for bit
    uint32_t n_nodes;
    float    cap;       // (float)history_cap, 0: none
};

inline TpMotionParams tp_motion_setup(const RtuTemporalDesc& d, const RtuFrameDesc& prev, const RtuFrameDesc& cur, bool has_prev, uint32_t n_nodes,
                                      int32_t history_cap) {
    TpMotionParams M{};
    M.P = tp_setup(d, prev, cur, has_prev);
    M.same_cam = M.P.lookup == TP_LOOKUP_STATIC;
    if (has_prev) M.P.lookup = TP_LOOKUP_REPROJECT;
    M.n_nodes = n_nodes;
    M.cap = (float)history_cap;
    return M;
}

// What the gradient form needs beyond TpMotionParams: one lambda per stratum, sw = ceil(width / TP_STRATUM) strata per row (host
// memory in the host form, device memory in the kernel); nullptr: no pixel is capped.
struct TpGradientParams {
    TpMotionParams M;
    const float*   lambda;
    int32_t        sw;
};

// What the sparse form needs beyond TpMotionParams: the shaded sample and the owner of every block (sw = ceil(width / block) blocks
// per row) in place of an image of samples, and the plane its holes are marked in (host memory in the host form, device memory in the
// kernel).
struct TpSparseParams {
    TpMotionParams  M;
    const float4*   rgbt;
    const uint32_t* owner;
    uint8_t*        hole;
    int32_t         block, sw;
};

// the words of an RtuNodeMotion that are read, in registers: the caller loads them (the kernel with 16-byte loads, the host form from
// a table of any alignment)
struct TpMotion {
    float    m[12], g[9];
    uint32_t flags;
};

RTU_HD TpMotion tp_motion_identity() {
    TpMotion T;
    for (int i = 0; i < 12; i++) T.m[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    for (int i = 0; i < 9; i++) T.g[i] = (i % 4 == 0) ? 1.0f : 0.0f;
    T.flags = RTU_MOTION_STATIC;
    return T;
}

// the index of a hit's node in a table of n_nodes entries, or -1: not a hit, node < 0, node >= n_nodes
RTU_HD int32_t tp_motion_index(const float4& hit0, uint32_t n_nodes) {
    union { float f; uint32_t u; } flags, node;
    flags.f = hit0.z;
    node.f = hit0.y;
    return ((flags.u & RTU_RAY_HIT) != 0 && node.u < n_nodes && node.u < 0x80000000u) ? (int32_t)node.u : -1;
}

// the table entry of a pixel (k >= 0) or the identity; 16-byte loads: the table is 16-byte aligned and an entry is 96 B
__device__ inline TpMotion tp_load_motion(const RtuNodeMotion* __restrict__ motion, int32_t k) {
    TpMotion T = tp_motion_identity();
    if (k >= 0) {
        const float4* e = reinterpret_cast<const float4*>(motion + k);
        const float4 a = e[0], b = e[1], c = e[2], d = e[3], f = e[4], g = e[5];
        union { float f; uint32_t u; } fl;
        fl.f = g.y;
        T.m[0] = a.x; T.m[1] = a.y; T.m[2] = a.z; T.m[3] = a.w; T.m[4] = b.x; T.m[5] = b.y; T.m[6] = b.z; T.m[7] = b.w;
        T.m[8] = c.x; T.m[9] = c.y; T.m[10] = c.z; T.m[11] = c.w;
        T.g[0] = d.x; T.g[1] = d.y; T.g[2] = d.z; T.g[3] = d.w; T.g[4] = f.x; T.g[5] = f.y; T.g[6] = f.z; T.g[7] = f.w; T.g[8] = g.x;
        T.flags = fl.u;
    }
    return T;
}

// Where the surface point of a pixel was in the previous scene: Pm, Nm by the pixel's table entry T (tp_motion_identity() when in_table
// is false). Returns whether the pixel may look its history up at all.
RTU_HD bool tp_moved_point(bool in_table, const TpMotion& T, const f3& Pp, const f3& Np, f3& Pm, f3& Nm) {
    const bool is_static = (T.flags & RTU_MOTION_STATIC) != 0;
    const f3 pm = mk3(dot3(mk3(T.m[0], T.m[1], T.m[2]), Pp) + T.m[3], dot3(mk3(T.m[4], T.m[5], T.m[6]), Pp) + T.m[7],
                      dot3(mk3(T.m[8], T.m[9], T.m[10]), Pp) + T.m[11]);
    const f3 q = mk3(dot3(mk3(T.g[0], T.g[1], T.g[2]), Np), dot3(mk3(T.g[3], T.g[4], T.g[5]), Np), dot3(mk3(T.g[6], T.g[7], T.g[8]), Np));
    const float len = sqrtf(dot3(q, q));
    const f3 nm = mk3(q.x / len, q.y / len, q.z / len);
    const bool fin = tp_finite(pm.x) && tp_finite(pm.y) && tp_finite(pm.z) && tp_finite(nm.x) && tp_finite(nm.y) && tp_finite(nm.z);
    Pm = is_static ? Pp : pm;
    Nm = is_static ? Np : nm;
    return in_table && (T.flags & RTU_MOTION_RESET) == 0 && (is_static || fin);
}

// ---- deforming meshes (include/rtu_render.h "Temporal accumulation on deforming meshes") ----------------------------------------------
// What the deform forms read besides the table: per mesh the connectivity and the PREVIOUS vertices and normals, per node its mesh
// (host memory in the host forms, device memory in the kernels).
struct TpDeformMesh {
    const uint32_t* f;
    const uint32_t* fn;
    const float*    v;   // previous positions
    const float*    vn;  // previous normals
    uint32_t        nf, reserved;
};
struct TpDeformScene {
    const TpDeformMesh* meshes;
    const int32_t*      node_mesh;  // n_nodes entries: RtuNode.mesh_id
    uint32_t            n_meshes, reserved;
};

// cyTriMesh::Interpolate as the walks state it (interp, rtu_intersect.h): (a[i0] bc0 + a[i1] bc1) + a[i2] bc2
RTU_HD f3 tp_interp(const float* arr, const uint32_t* idx, const f3& bc) {
    return (ld3(arr + 3 * (size_t)idx[0]) * bc.x + ld3(arr + 3 * (size_t)idx[1]) * bc.y) + ld3(arr + 3 * (size_t)idx[2]) * bc.z;
}

// What a pixel of the deform forms carries through its table entry T, and whether it may look its history up: for a DEFORM entry
// the point x and the (unnormalised) normal n of its surface record (s0, s1: the two float4 of an RtuRaySurface) over the previous
// vertices — false when the record is not of the node's mesh or its face is out of range —, else the hit's own Pp, Np. T.flags loses
// RTU_MOTION_STATIC where it has RTU_MOTION_DEFORM: such a pixel always reprojects. k: the pixel's table index (>= 0).
RTU_HD bool tp_deform_source(const TpDeformScene& D, int32_t k, TpMotion& T, const float4& s0, const float4& s1, const f3& Pp, const f3& Np, f3& x, f3& n) {
    x = Pp;
    n = Np;
    if (k < 0 || (T.flags & RTU_MOTION_DEFORM) == 0) return true;
    T.flags &= ~RTU_MOTION_STATIC;
    union { float f; int32_t i; } mesh, face;
    mesh.f = s0.x;
    face.f = s0.y;
    const int32_t nm = D.node_mesh[k];
    if (nm < 0 || (uint32_t)nm >= D.n_meshes || mesh.i != nm) return false;
    const TpDeformMesh& M = D.meshes[nm];
    if (face.i < 0 || (uint32_t)face.i >= M.nf) return false;
    const f3 bc = mk3(s0.z, s0.w, s1.x);
    x = tp_interp(M.v, M.f + 3 * (size_t)face.i, bc);
    n = tp_interp(M.vn, M.fn + 3 * (size_t)face.i, bc);
    return true;
}

// The previous-image coordinates of world point Pm: false unless s is finite and > 0.
RTU_HD bool tp_project(const TpParams& P, const f3& Pm, float& fx, float& fy) {
    const f3 pos = ld3(P.pos), nrm = ld3(P.nrm);
    const f3 D = Pm - pos;
    const float s = P.num / dot3(D, nrm);
    const f3 Q = (pos + D * s) - ld3(P.origin);
    fx = dot3(Q, ld3(P.u)) / P.uu - 0.5f;
    fy = dot3(Q, ld3(P.v)) / P.vv - 0.5f;
    return tp_finite(s) && s > 0.0f;
}

// ---- the projection: a compile-time policy of tp_pixel and tp_tap ----------------------------------------------------------------------
// project(): the previous-image coordinates of a world point, or false; column(): the column a tap at column qx reads (a tap whose
// column is then outside the image is dropped). TpPinhole, the default, is the camera of TpParams; TpSensorProj<MODEL> is a sensor of
// "Temporal accumulation for sensors", whose equirectangular columns WRAP: -1 is the last column, width is column 0.
struct TpPinhole {
    RTU_HD bool project(const TpParams& P, const f3& Pm, float& fx, float& fy) const { return tp_project(P, Pm, fx, fy); }
    RTU_HD int  column(const TpParams&, int qx) const { return qx; }
};
template <int MODEL>
struct TpSensorProj {
    const RtuSensorDesc& prev;  // the PREVIOUS sensor
    RTU_HD bool project(const TpParams&, const f3& Pm, float& fx, float& fy) const { return sensor_project<MODEL>(prev, Pm, fx, fy); }
    RTU_HD int  column(const TpParams& P, int qx) const {
        if (MODEL != RTU_SENSOR_EQUIRECT) return qx;
        return qx < 0 ? qx + P.width : (qx >= P.width ? qx - P.width : qx);
    }
};

inline bool tp_same_sensor(const RtuSensorDesc& a, const RtuSensorDesc& b) {
    union { float f; uint32_t u; } x, y;
    if (a.model != b.model || a.width != b.width || a.height != b.height) return false;
    const auto same = [&](float fa, float fb) { x.f = fa; y.f = fb; return x.u == y.u; };
    for (int k = 0; k < 3; k++)
        if (!same(a.pos[k], b.pos[k]) || !same(a.right[k], b.right[k]) || !same(a.up[k], b.up[k]) || !same(a.forward[k], b.forward[k])) return false;
    if (a.model == RTU_SENSOR_FISHEYE && !same(a.fov_deg, b.fov_deg)) return false;
    if (a.model == RTU_SENSOR_ORTHO && (!same(a.extent[0], b.extent[0]) || !same(a.extent[1], b.extent[1]))) return false;
    return true;
}

// TpParams of the sensor forms: the camera fields stay zero (TpSensorProj reads the previous sensor itself). No lookup without a
// previous history or between sensors of another model or size.
inline TpParams tp_sensor_setup(const RtuTemporalDesc& d, const RtuSensorDesc& prev, const RtuSensorDesc& cur, bool has_prev) {
    TpParams p{};
    p.width = d.width;
    p.height = d.height;
    const bool comparable = has_prev && prev.model == cur.model && prev.width == cur.width && prev.height == cur.height;
    p.lookup = !comparable ? TP_LOOKUP_NONE : (tp_same_sensor(prev, cur) ? TP_LOOKUP_STATIC : TP_LOOKUP_REPROJECT);
    p.max_history = (float)d.max_history;
    p.sigma_plane = d.sigma_plane;
    p.normal_min = d.normal_min;
    return p;
}

// l(e) of a demodulated colour: what the moments are taken of
RTU_HD float vr_lum(const f3& e) { return (0.2126f * e.x + 0.7152f * e.y) + 0.0722f * e.z; }

// ---- the accumulator: one function for the three forms ---------------------------------------------------------------------------
// MOVING: the hit point is carried through its node's table entry before the lookup, and the history taken over is capped
// (TpMotionParams); else the scene is at rest (TpParams). MOMENTS: the history has the fourth plane M. GRADIENT (with both): the
// history taken over is capped once more, by the lambda of the pixel's stratum (TpGradientParams). SPARSE (with MOVING and MOMENTS):
// only the pixel its block owns has a sample (TpSparseParams); every other pixel keeps its history.
template <bool MOVING, bool GRADIENT = false, bool SPARSE = false>
using TpArgs = typename std::conditional<
    SPARSE, TpSparseParams,
    typename std::conditional<GRADIENT, TpGradientParams, typename std::conditional<MOVING, TpMotionParams, TpParams>::type>::type>::type;
RTU_HD const TpParams& tp_base(const TpParams& p) { return p; }
RTU_HD const TpParams& tp_base(const TpMotionParams& m) { return m.P; }
RTU_HD const TpParams& tp_base(const TpGradientParams& g) { return g.M.P; }
RTU_HD const TpParams& tp_base(const TpSparseParams& s) { return s.M.P; }
RTU_HD const TpMotionParams& tp_motion(const TpMotionParams& m) { return m; }
RTU_HD const TpMotionParams& tp_motion(const TpGradientParams& g) { return g.M; }
RTU_HD const TpMotionParams& tp_motion(const TpSparseParams& s) { return s.M; }

// the weighted sums over the accepted taps of a lookup: E.rgb, E.n, the weights, and with MOMENTS M.xy
struct TpSums {
    f3    acc;
    float n, w, m1, m2;
};

// One tap of pixel p's lookup at pixel (qx, qy) of the previous history h (its planes) with weight w: where it is ACCEPTED, it is added
// to S. Pp, Np: p's point and normal as they were in the previous scene.
template <bool MOMENTS, class PROJ = TpPinhole>
RTU_HD void tp_tap(const TpParams& P, const float4* const* h, int qx, int qy, float w, const f3& Np, const f3& Pp, uint32_t node, float plane_max,
                   TpSums& S, const PROJ& proj = PROJ()) {
    qx = proj.column(P, qx);
    if (qx < 0 || qy < 0 || qx >= P.width || qy >= P.height) return;
    const size_t q = (size_t)qy * (size_t)P.width + (size_t)qx;
    const float4 Eq = h[0][q], Pq = h[1][q], Nq = h[2][q];
    union { float f; uint32_t u; } nb;
    nb.f = Nq.w;
    if (!(Eq.w > 0.0f) || nb.u != node) return;
    if (!(dot3(Np, mk3(Nq.x, Nq.y, Nq.z)) >= P.normal_min)) return;
    if (!(fabsf(dot3(Np, mk3(Pq.x, Pq.y, Pq.z) - Pp)) <= plane_max)) return;
    S.acc = S.acc + mk3(Eq.x, Eq.y, Eq.z) * w;
    S.n = S.n + Eq.w * w;
    S.w = S.w + w;
    if (MOMENTS) {
        const float4 Mq = h[3][q];
        S.m1 = S.m1 + Mq.x * w;
        S.m2 = S.m2 + Mq.y * w;
    }
}

// Pixel (x, y): h the three (MOMENTS: four) planes of the previous history (not read with TP_LOOKUP_NONE), hit the three float4 of its
// RtuRayHit; MOVING: in_table / T as for tp_moved_point (else neither is read). out: its pixel of the accumulated image; o: its pixel
// of the planes of the new history, all written after every read. A.lookup is wave-uniform without MOVING; with it, whether a pixel
// takes no, one or four taps is its own matter. SPARSE: `owner` — the pixel is the one its block shades this frame and rgbz is that
// sample; for every other pixel nothing of rgbz reaches an output — and *hole, the pixel's mark in the hole plane (without SPARSE
// neither is used).
// DEFORM (with MOVING): what is carried through T is src[0], src[1] of tp_deform_source in place of the hit's point and normal, and
// there is no lookup unless src_ok.
template <bool MOVING, bool MOMENTS, bool GRADIENT = false, bool SPARSE = false, class PROJ = TpPinhole, bool DEFORM = false>
RTU_HD void tp_pixel(const TpArgs<MOVING, GRADIENT, SPARSE>& A, bool in_table, const TpMotion& T, const float4* const* h, int x, int y, const float4& rgbz,
                     const float4* hit, const float4& albedo, float4& out, float4* o, bool owner = true, uint8_t* hole = nullptr,
                     const PROJ& proj = PROJ(), const f3* src = nullptr, bool src_ok = true) {
    static_assert(!DEFORM || (MOVING && !GRADIENT && !SPARSE), "the deform forms are the motion and the moments form");
    static_assert(!GRADIENT || (MOVING && MOMENTS), "the gradient form is a moments form");
    static_assert(!SPARSE || (MOVING && MOMENTS && !GRADIENT), "the sparse form is a moments form");
    const TpParams& P = tp_base(A);
    union { float f; uint32_t u; } flags, node;
    flags.f = hit[0].z;
    node.f = hit[0].y;
    const bool valid = (flags.u & RTU_RAY_HIT) != 0;
    const f3 d = dn_demod(albedo);
    const f3 e_cur = mk3(rgbz.x / d.x, rgbz.y / d.y, rgbz.z / d.z);
    const f3 Pp = mk3(hit[1].x, hit[1].y, hit[1].z), Np = mk3(hit[2].x, hit[2].y, hit[2].z);
    const float plane_max = P.sigma_plane * hit[0].x;

    f3 Pm = Pp, Nm = Np;
    bool look = valid && P.lookup != TP_LOOKUP_NONE, one_tap = valid && P.lookup == TP_LOOKUP_STATIC;
    if constexpr (MOVING) {
        if constexpr (DEFORM) look = tp_moved_point(in_table && src_ok, T, src[0], src[1], Pm, Nm) && look;
        else look = tp_moved_point(in_table, T, Pp, Np, Pm, Nm) && look;
        one_tap = look && tp_motion(A).same_cam != 0 && (T.flags & RTU_MOTION_STATIC) != 0;
    }

    TpSums S = {mk3(0.0f, 0.0f, 0.0f), 0.0f, 0.0f, 0.0f, 0.0f};
    f3 e_prev = mk3(0.0f, 0.0f, 0.0f);
    float n_prev = 0.0f, m1_prev = 0.0f, m2_prev = 0.0f;
    if (one_tap) {
        tp_tap<MOMENTS, PROJ>(P, h, x, y, 1.0f, Nm, Pm, node.u, plane_max, S, proj);
    } else if (look) {
        float fx, fy;
        // (a NaN fails; tested before any conversion)
        if (proj.project(P, Pm, fx, fy) && fx >= -1.0f && fx < (float)P.width && fy >= -1.0f && fy < (float)P.height) {
            const float flx = floorf(fx), fly = floorf(fy);
            const int x0 = (int)flx, y0 = (int)fly;
            const float wx = fx - flx, wy = fy - fly;
            const float ux = 1.0f - wx, uy = 1.0f - wy;
            tp_tap<MOMENTS, PROJ>(P, h, x0, y0, ux * uy, Nm, Pm, node.u, plane_max, S, proj);
            tp_tap<MOMENTS, PROJ>(P, h, x0 + 1, y0, wx * uy, Nm, Pm, node.u, plane_max, S, proj);
            tp_tap<MOMENTS, PROJ>(P, h, x0, y0 + 1, ux * wy, Nm, Pm, node.u, plane_max, S, proj);
            tp_tap<MOMENTS, PROJ>(P, h, x0 + 1, y0 + 1, wx * wy, Nm, Pm, node.u, plane_max, S, proj);
        }
    }
    if (S.w > 0.01f) {
        e_prev = mk3(S.acc.x / S.w, S.acc.y / S.w, S.acc.z / S.w);
        n_prev = S.n / S.w;
        if (MOMENTS) {
            m1_prev = S.m1 / S.w;
            m2_prev = S.m2 / S.w;
        }
    }
    if constexpr (MOVING)
        if (tp_motion(A).cap > 0.0f && n_prev > 0.0f) n_prev = smin(n_prev, tp_motion(A).cap);
    if constexpr (GRADIENT) {  // the weight of the new sample is not below lambda; lambda >= 1 starts the pixel over
        const float lambda = A.lambda ? A.lambda[(size_t)(y / TP_STRATUM) * (size_t)A.sw + (size_t)(x / TP_STRATUM)] : 0.0f;
        if (lambda > 0.0f && n_prev > 0.0f) n_prev = smin(n_prev, lambda < 1.0f ? 1.0f / lambda - 1.0f : 0.0f);
        if (n_prev == 0.0f) {  // (lambda >= 1) as a pixel that found no history
            e_prev = mk3(0.0f, 0.0f, 0.0f);
            m1_prev = 0.0f;
            m2_prev = 0.0f;
        }
    }

    // else the sample is not accumulated; a pixel that is not its block's owner has none
    const bool finite = (!SPARSE || owner) && tp_finite(rgbz.x) && tp_finite(rgbz.y) && tp_finite(rgbz.z);
    const bool fresh = n_prev == 0.0f;
    const float n_blend = smin(n_prev + 1.0f, P.max_history);
    const float a = 1.0f / n_blend;
    const f3 e_blend = e_prev + (e_cur - e_prev) * a;
    const f3 e = !finite ? e_prev : (fresh ? e_cur : e_blend);
    const float n = !finite ? n_prev : (fresh ? 1.0f : n_blend);
    const bool keep = valid && (finite || !fresh);  // the pixel has an accumulated colour; else its input passes through
    if (MOMENTS) {  // l l finite (so l is) or the sample leaves the moments as they were — zeros for a fresh pixel
        const float l = vr_lum(e_cur), l2 = l * l;
        const bool usable = finite && tp_finite(l2);
        const float m1_blend = m1_prev + (l - m1_prev) * a, m2_blend = m2_prev + (l2 - m2_prev) * a;
        const float m1 = !usable ? m1_prev : (fresh ? l : m1_blend);
        const float m2 = !usable ? m2_prev : (fresh ? l2 : m2_blend);
        o[3] = keep ? make_float4(m1, m2, 0.0f, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    if (!valid) node.u = 0xFFFFFFFFu;  // node -1
    out = keep ? make_float4(e.x * d.x, e.y * d.y, e.z * d.z, rgbz.w) : rgbz;
    if constexpr (SPARSE) {  // no sample of its own: the depth is the guides', and without an accumulated colour the pixel is a hole
        if (!owner) {
            const float z = valid ? hit[0].x : RTU_BIGFLOAT;
            out = keep ? make_float4(e.x * d.x, e.y * d.y, e.z * d.z, z) : make_float4(0.0f, 0.0f, 0.0f, z);
        }
        *hole = (!owner && !keep) ? 1 : 0;
    }
    o[0] = keep ? make_float4(e.x, e.y, e.z, n) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    o[1] = valid ? make_float4(Pp.x, Pp.y, Pp.z, hit[0].x) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    o[2] = valid ? make_float4(Np.x, Np.y, Np.z, node.f) : make_float4(0.0f, 0.0f, 0.0f, node.f);
}
// the motion vector of a pixel: {fx, fy, 1, 0} or zeros
RTU_HD float4 tp_motion_vector(const TpParams& P, bool in_table, const TpMotion& T, const float4* hit) {
    f3 Pm, Nm;
    const f3 Pp = mk3(hit[1].x, hit[1].y, hit[1].z), Np = mk3(hit[2].x, hit[2].y, hit[2].z);
    (void)tp_moved_point(in_table, T, Pp, Np, Pm, Nm);
    float fx, fy;
    const bool ok = tp_project(P, Pm, fx, fy) && in_table && (T.flags & RTU_MOTION_RESET) == 0 && tp_finite(Pm.x) && tp_finite(Pm.y) && tp_finite(Pm.z);
    return ok ? make_float4(fx, fy, 1.0f, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// ... of the deform forms: Pm from (src[0], src[1]) of tp_deform_source
RTU_HD float4 tp_motion_vector_deform(const TpParams& P, bool in_table, const TpMotion& T, const f3* src, bool src_ok) {
    f3 Pm, Nm;
    (void)tp_moved_point(in_table, T, src[0], src[1], Pm, Nm);
    float fx, fy;
    const bool ok = tp_project(P, Pm, fx, fy) && in_table && src_ok && (T.flags & RTU_MOTION_RESET) == 0 && tp_finite(Pm.x) && tp_finite(Pm.y) && tp_finite(Pm.z);
    return ok ? make_float4(fx, fy, 1.0f, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// RTU_OK or RTU_ERR_ARG: the rules of RtuTemporalDesc (include/rtu_render.h)
int rtu_temporal_check_desc(const RtuTemporalDesc* d);
// RTU_OK or RTU_ERR_ARG: the rules of RtuSparseDesc (rtu_sparse.hip)
int rtu_sparse_check_desc(const RtuSparseDesc* d);
// RTU_OK or RTU_ERR_ARG: history_cap 0 .. 65535; with a host table, its reserved words 0 and its flags known
// (allow_deform: RTU_MOTION_DEFORM is a known flag — the deform forms)
int rtu_temporal_check_motion(const RtuNodeMotion* h_motion_or_null, uint32_t n_nodes, int32_t history_cap, bool allow_deform = false);
// mv[i] = the motion vector of pixel i
int rtu_launch_motion_vectors(const TpParams& p, uint32_t n_nodes, const float4* hits, const RtuNodeMotion* d_motion, float4* mv, hipStream_t stream);

// The accumulator on the device: rgbz, albedo, rgbz_out [width * height] float4, hits [width * height] RtuRayHit, hist_prev (nullptr
// with TP_LOOKUP_NONE) and hist_out three planes of width * height float4 each. rgbz_out == rgbz is allowed; hist_out does not overlap
// hist_prev. Pointers 16-byte aligned and desc checked by the caller. Returns a hipError_t as int. Asynchronous on `stream`.
int rtu_launch_temporal(const TpParams& p, const float4* rgbz, const float4* hits, const float4* albedo, const float4* hist_prev, float4* hist_out,
                        float4* rgbz_out, hipStream_t stream);
// The motion form: d_motion n_nodes entries, 16-byte aligned (nullptr allowed with n_nodes == 0). The moments form: that with histories
// of four planes.
int rtu_launch_temporal_motion(const TpMotionParams& m, const float4* rgbz, const float4* hits, const float4* albedo, const float4* hist_prev,
                               float4* hist_out, float4* rgbz_out, const RtuNodeMotion* d_motion, hipStream_t stream);
int rtu_launch_temporal_moments(const TpMotionParams& m, const float4* rgbz, const float4* hits, const float4* albedo, const float4* hist_prev,
                                float4* hist_out, float4* rgbz_out, const RtuNodeMotion* d_motion, hipStream_t stream);
// The deform forms (k_temporal_deform<MOMENTS>): the motion / moments form with the surface records of the frame (two float4 per
// pixel) and D, whose arrays are device memory.
int rtu_launch_temporal_deform(const TpMotionParams& m, bool moments, const TpDeformScene& D, const float4* rgbz, const float4* hits, const float4* albedo,
                               const float4* surface, const float4* hist_prev, float4* hist_out, float4* rgbz_out, const RtuNodeMotion* d_motion,
                               hipStream_t stream);
int rtu_launch_motion_vectors_deform(const TpParams& p, uint32_t n_nodes, const TpDeformScene& D, const float4* hits, const float4* surface,
                                     const RtuNodeMotion* d_motion, float4* mv, hipStream_t stream);
// The gradient form: the moments form with g.lambda, device memory (nullptr: the moments form's bits).
int rtu_launch_temporal_capped(const TpGradientParams& g, const float4* rgbz, const float4* hits, const float4* albedo, const float4* hist_prev,
                               float4* hist_out, float4* rgbz_out, const RtuNodeMotion* d_motion, hipStream_t stream);
// The sparse form: the moments form whose samples are s.rgbt / s.owner, one per block; s.hole [width * height] is written.
int rtu_launch_temporal_sparse(const TpSparseParams& s, const float4* hits, const float4* albedo, const float4* hist_prev, float4* hist_out,
                               float4* rgbz_out, const RtuNodeMotion* d_motion, hipStream_t stream);
// The sensor forms (k_temporal_sensor<MODEL, MOMENTS>, MODEL = prev.model): p of tp_sensor_setup; the scene is at rest, there is no
// table. The histories have three planes, with `moments` four.
int rtu_launch_temporal_sensor(const TpParams& p, const RtuSensorDesc& prev, bool moments, const float4* rgbz, const float4* hits, const float4* albedo,
                               const float4* hist_prev, float4* hist_out, float4* rgbz_out, hipStream_t stream);
// n_out[i] = the history length of pixel i (E.w of `hist`), or 0 everywhere with hist == nullptr
int rtu_launch_temporal_history(const float4* hist, float* n_out, size_t pixels, hipStream_t stream);

#endif
