// rtu_irradiance.h — the arithmetic of the screen-space irradiance map (include/rtu_render.h "Irradiance map"), host + device, and the
// launch interface of its kernels (rtu_irradiance.hip, render_rays6.hip / render_rays7.hip), called by rtu_capi.hip.
//   irr_grid / irr_pass / irr_pass_point   the grid of a frame and the points a pass visits, in the order it visits them
//   irr_neighbours / irr_estimate          which four earlier points a visited point is estimated from, and whether their average will do
//   irr_point_ray                          the pinhole ray through a grid point (a pixel corner)
//   irr_sample                             the bilinear lookup at an image position
// The floating-point expressions round once per operation: the translation units that include this header are compiled with
// -ffp-contract=off and IEEE divides, so the host forms and the kernels give the same bits.
#ifndef RTU_IRRADIANCE_H_INCLUDED
#define RTU_IRRADIANCE_H_INCLUDED

#include "rtu_camrays.h"

struct IrrGrid {
    uint32_t gw, gh;     // points per row, rows
    uint32_t scale;      // s = 2^-max_subdiv: pixels between neighbouring points
    uint32_t levels;     // max_subdiv - min_subdiv; 1 + 2 * levels passes
};

// Pass p: phase 0 the coarse grid (p == 0), 1 the cell centres and 2 the edge midpoints of level (p + 1) / 2, whose cells have
// `skip` points between their corners; half = skip / 2. A pass visits its points row by row, so in rising grid index.
struct IrrPass {
    uint32_t gw, gh, phase, skip, half;
    uint32_t nxe, nxo;   // points per visited row: phase 2 alternates rows that start at `half` (nxe) and at 0 (nxo); else nxe only
    uint32_t rows;       // visited rows
    uint32_t count;      // visited points
};

struct IrrThresholds {
    float color[3], z, n;
};

struct IrrCam {
    float    cam_pos[3], origin[3], u[3], v[3];
    float    scale;      // (float)s
    uint32_t gw;
};

// the listed points of (a chunk of) a pass, for k_irr_roots: chain j * samples + m belongs to point list[j]
struct IrrRoots {
    IrrCam          cam;
    const uint32_t* list;
    uint32_t        n_points, samples, first_sample;
};

// RTU_OK, RTU_ERR_ARG or RTU_ERR_UNSUPPORTED: the rules of RtuIrradianceDesc for a width x height image
int rtu_irradiance_check(const RtuIrradianceDesc* d, int width, int height, IrrGrid* g);

RTU_HD IrrPass irr_pass(const IrrGrid& g, uint32_t p) {
    IrrPass q;
    q.gw = g.gw;
    q.gh = g.gh;
    q.phase = p == 0u ? 0u : 2u - (p & 1u);
    const uint32_t level = (p + 1u) / 2u;  // 0 for the coarse pass
    q.skip = 1u << (g.levels - (level ? level - 1u : 0u));
    q.half = q.skip / 2u;
    const uint32_t from0_x = (g.gw - 1u) / q.skip + 1u, from0_y = (g.gh - 1u) / q.skip + 1u;
    const uint32_t fromh_x = g.gw > q.half ? (g.gw - 1u - q.half) / q.skip + 1u : 0u, fromh_y = g.gh > q.half ? (g.gh - 1u - q.half) / q.skip + 1u : 0u;
    if (q.phase == 0u) {
        q.nxe = from0_x; q.nxo = 0u; q.rows = from0_y; q.count = from0_x * from0_y;
    } else if (q.phase == 1u) {
        q.nxe = fromh_x; q.nxo = 0u; q.rows = fromh_y; q.count = fromh_x * fromh_y;
    } else {
        q.nxe = fromh_x; q.nxo = from0_x;
        q.rows = (g.gh - 1u) / q.half + 1u;  // rows 0, half, 2 half, ...: the even ones start at half, the odd ones at 0
        q.count = ((q.rows + 1u) / 2u) * q.nxe + (q.rows / 2u) * q.nxo;
    }
    return q;
}

// the k-th point pass q visits, k < q.count
RTU_HD void irr_pass_point(const IrrPass& q, uint32_t k, uint32_t& x, uint32_t& y) {
    if (q.phase == 0u) {
        y = (k / q.nxe) * q.skip;
        x = (k % q.nxe) * q.skip;
    } else if (q.phase == 1u) {
        y = q.half + (k / q.nxe) * q.skip;
        x = q.half + (k % q.nxe) * q.skip;
    } else {
        const uint32_t per = q.nxe + q.nxo, pair = k / per, rem = k - pair * per;
        if (rem < q.nxe) { y = (2u * pair) * q.half; x = q.half + rem * q.skip; }
        else { y = (2u * pair + 1u) * q.half; x = (rem - q.nxe) * q.skip; }
    }
}

// The four points (x, y) may be estimated from, in the order their records are added; false: the point is always computed (the
// coarse pass; a cell that the grid cuts off; in the edge pass a point of the first row or column as well).
RTU_HD bool irr_neighbours(const IrrPass& q, uint32_t x, uint32_t y, uint32_t idx[4]) {
    if (q.phase == 0u) return false;
    const uint32_t x2 = x + q.half, y2 = y + q.half;
    if (!(x2 < q.gw && y2 < q.gh)) return false;
    if (q.phase == 1u) {
        const uint32_t x1 = x - q.half, y1 = y - q.half;
        idx[0] = y1 * q.gw + x1; idx[1] = y1 * q.gw + x2; idx[2] = y2 * q.gw + x1; idx[3] = y2 * q.gw + x2;
        return true;
    }
    if (!(x > 0u && y > 0u)) return false;
    const uint32_t x1 = x - q.half, y1 = y - q.half;
    idx[0] = y1 * q.gw + x; idx[1] = y * q.gw + x1; idx[2] = y * q.gw + x2; idx[3] = y2 * q.gw + x;
    return true;
}

RTU_HD float irr_avg4(float a, float b, float c, float d) { return (((a + b) + c) + d) * 0.25f; }

// the average of the four records {E.rgb, z} {N.xyz, -}, and whether it is similar to each of them
RTU_HD bool irr_estimate(const IrrThresholds& t, const float4* rec, const uint32_t idx[4], float4& avgA, float4& avgB) {
    float4 A[4], B[4];
    for (int k = 0; k < 4; k++) { A[k] = rec[2 * (size_t)idx[k]]; B[k] = rec[2 * (size_t)idx[k] + 1]; }
    avgA = make_float4(irr_avg4(A[0].x, A[1].x, A[2].x, A[3].x), irr_avg4(A[0].y, A[1].y, A[2].y, A[3].y), irr_avg4(A[0].z, A[1].z, A[2].z, A[3].z),
                       irr_avg4(A[0].w, A[1].w, A[2].w, A[3].w));
    avgB = make_float4(irr_avg4(B[0].x, B[1].x, B[2].x, B[3].x), irr_avg4(B[0].y, B[1].y, B[2].y, B[3].y), irr_avg4(B[0].z, B[1].z, B[2].z, B[3].z), 0.0f);
    bool ok = true;
    for (int k = 0; k < 4; k++) {
        const bool similar = fabsf(avgA.x - A[k].x) < t.color[0] && fabsf(avgA.y - A[k].y) < t.color[1] && fabsf(avgA.z - A[k].z) < t.color[2] &&
                             fabsf(avgA.w - A[k].w) < t.z && dot3(mk3(avgB.x, avgB.y, avgB.z), mk3(B[k].x, B[k].y, B[k].z)) > t.n;
        ok = ok && similar;
    }
    return ok;
}

// grid point `point` sits at the image position (x s, y s): the ray from the pinhole through it, by rtu_camera_rays' expressions
RTU_HD void irr_point_ray(const IrrCam& c, uint32_t point, f3& org, f3& dir) {
    const uint32_t y = point / c.gw, x = point - y * c.gw;
    const float sx = (float)x * c.scale, sy = (float)y * c.scale;
    const f3 cp = (ld3(c.origin) + ld3(c.u) * sx) + ld3(c.v) * sy;
    org = ld3(c.cam_pos);
    dir = norm3(cp - org);
}

RTU_HD float irr_lerp(float a, float b, float f) { return a * (1.0f - f) + b * f; }
RTU_HD float4 irr_lerp4(const float4& a, const float4& b, float f) {
    return make_float4(irr_lerp(a.x, b.x, f), irr_lerp(a.y, b.y, f), irr_lerp(a.z, b.z, f), irr_lerp(a.w, b.w, f));
}

// the record at image position (px, py): truncate, clamp to the last row and column, interpolate in x, then in y. A negative or
// NaN coordinate is taken as 0.
RTU_HD void irr_sample(const float4* rec, uint32_t gw, uint32_t gh, uint32_t scale, float px, float py, float4& outA, float4& outB) {
    const float iskip = 1.0f / (float)scale;
    float xx = px * iskip, yy = py * iskip;
    if (!(xx > 0.0f)) xx = 0.0f;
    if (!(yy > 0.0f)) yy = 0.0f;
    uint32_t ix = xx < 4.0e9f ? (uint32_t)xx : 4000000000u, iy = yy < 4.0e9f ? (uint32_t)yy : 4000000000u;
    const float fx = xx - (float)ix, fy = yy - (float)iy;
    uint32_t ix2 = ix + 1u, iy2 = iy + 1u;
    if (ix >= gw) ix = ix2 = gw - 1u;
    else if (ix2 >= gw) ix2 = gw - 1u;
    if (iy >= gh) iy = iy2 = gh - 1u;
    else if (iy2 >= gh) iy2 = gh - 1u;
    const size_t i0 = (size_t)iy * gw + ix, i1 = (size_t)iy * gw + ix2, i2 = (size_t)iy2 * gw + ix, i3 = (size_t)iy2 * gw + ix2;
    outA = irr_lerp4(irr_lerp4(rec[2 * i0], rec[2 * i1], fx), irr_lerp4(rec[2 * i2], rec[2 * i3], fx), fy);
    outB = irr_lerp4(irr_lerp4(rec[2 * i0 + 1], rec[2 * i1 + 1], fx), irr_lerp4(rec[2 * i2 + 1], rec[2 * i3 + 1], fx), fy);
}

// ---- the kernels of rtu_irradiance.hip; every launch function is asynchronous on `stream` and returns a hipError_t as int ----
// words of scratch a pass over at most `points` visited points needs (16-byte aligned)
size_t rtu_irr_scratch_words(size_t points);
// One pass up to its list: the visited points that can be estimated get their average and the byte 0, the others are listed in
// visiting order — list[0 .. *total) — through the allocation scan of rtu_steer.hip. scratch: rtu_irr_scratch_words(q.count) words.
int rtu_launch_irr_classify(const IrrPass& q, const IrrThresholds& t, float4* rec, uint8_t* computed, uint32_t* list, uint32_t* total, uint32_t* scratch,
                            hipStream_t stream);
// E = the sum of the `samples` values c of point j in their order, divided by (float)samples; z and N from the point's depth-0 chain
// records; the byte 1. c: {c, t} per chain (k_gather_amb); gi_h: the chain records of n_points * samples chains.
int rtu_launch_irr_store(const uint32_t* list, uint32_t n_points, uint32_t samples, const float4* c, const float4* gi_h, float4* rec, uint8_t* computed,
                         hipStream_t stream);
// out[2 i], out[2 i + 1] = irr_sample at (xy[2 i], xy[2 i + 1])
int rtu_launch_irr_sample(const float4* rec, const IrrGrid& g, const float* xy, size_t n, float4* out, hipStream_t stream);
// amb[p] = {E, 0} of irr_sample at the centre (x + 0.5, y + 0.5) of every pixel p of a width x height image
int rtu_launch_irr_lookup_centres(const float4* rec, const IrrGrid& g, uint32_t width, uint32_t height, float4* amb, hipStream_t stream);

// ---- render_rays6.hip / render_rays7.hip (render_gather_impl.h) ----
struct DevScene;
int rtu_launch_gather_amb(const DevScene& s, const float4* gi_h, const float4* gi_res, uint32_t n, float4* out, hipStream_t stream);
int rtu_launch_amb_seed(float4* gi_h, float4* gi_res, const float4* amb, uint32_t n, hipStream_t stream);
int rtu_launch_irr_roots(const DevScene& s, const IrrRoots& r, uint32_t bvh_stack_needed, float4* gi_h, float4* out, hipStream_t stream);

#endif
