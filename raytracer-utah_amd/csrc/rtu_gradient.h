// rtu_gradient.h — the arithmetic of temporal gradients (include/rtu_render.h "Temporal gradients"), host + device, and the launch
// interface of its kernels (rtu_gradient.hip), called by rtu_capi_temporal.hip:
//   gr_owner       rtu_gradient_rays: the pixel a 3 x 3 stratum re-shades this frame (the ray itself is camera_sample_ray of rtu_camrays.h)
//   gr_luminance   rtu_sample_luminance: l(c / d) of a raw sample, what the next frame's gradients are taken against
//   gr_diff        rtu_temporal_gradient, first half: {num, den, noise, 0} of a stratum — its owner re-shaded with the previous frame's
//                  random numbers against what the previous frame saw where the accumulator looks that pixel's history up
//   gr_lambda      ... second half: the sums over the neighbouring strata and lambda
// The capped accumulator is tp_pixel<true, true, true> of rtu_temporal.h. Binary32, one rounding per operation: the translation units
// that include this header are compiled with -ffp-contract=off and IEEE divides and square roots, so the host forms and the kernels
// give the same bits.
#ifndef RTU_GRADIENT_H_INCLUDED
#define RTU_GRADIENT_H_INCLUDED

#include "rtu_camrays.h"
#include "rtu_temporal.h"

#define GR_MAX_RADIUS 3

inline int32_t gr_strata(int32_t pixels) { return (pixels + (TP_STRATUM - 1)) / TP_STRATUM; }

// ---- 1. owners -------------------------------------------------------------------------------------------------------------------
// the pixel (x, y) of stratum s = sx + sw * sy of a width x height image in frame frame_index: always inside the stratum and the image
RTU_HD void gr_owner(int32_t width, int32_t height, int32_t sw, uint32_t s, uint32_t frame_index, int& x, int& y) {
    const int32_t sy = (int32_t)(s / (uint32_t)sw), sx = (int32_t)(s - (uint32_t)sy * (uint32_t)sw);
    const uint32_t h = cs_mix32(s + 0x9e3779b9u * (frame_index + 1u));
    const int32_t rx = width - TP_STRATUM * sx, ry = height - TP_STRATUM * sy;
    x = TP_STRATUM * sx + (int32_t)((h >> 16) % (uint32_t)(rx < TP_STRATUM ? rx : TP_STRATUM));
    y = TP_STRATUM * sy + (int32_t)((h >> 24) % (uint32_t)(ry < TP_STRATUM ? ry : TP_STRATUM));
}

// ---- 2. the sample's luminance ---------------------------------------------------------------------------------------------------
// hit0 the first float4 of the pixel's RtuRayHit
RTU_HD float gr_luminance(const float4& rgbz, const float4& hit0, const float4& albedo) {
    union { float f; uint32_t u; } flags;
    flags.f = hit0.z;
    const bool ok = (flags.u & RTU_RAY_HIT) != 0 && tp_finite(rgbz.x) && tp_finite(rgbz.y) && tp_finite(rgbz.z);
    const f3 d = dn_demod(albedo);
    const float l = vr_lum(mk3(rgbz.x / d.x, rgbz.y / d.y, rgbz.z / d.z));
    return ok ? l : 0.0f;
}

// ---- 3. gradients and lambda -----------------------------------------------------------------------------------------------------
struct GrParams {
    TpMotionParams M;  // as the accumulator's of the same frame (M.cap is not read)
    int32_t sw, sh, radius;
    float   kappa;
};

// The gradient of the stratum whose owner is pixel (x, y): hit, albedo the owner's guides in the current frame, in_table / T as for
// tp_moved_point, h the four planes of the previous history and lum_prev the previous sample's luminance plane (neither read with
// TP_LOOKUP_NONE), c the shaded {r, g, b, t} of the gradient ray.
RTU_HD float4 gr_diff(const TpMotionParams& A, bool in_table, const TpMotion& T, const float4* const* h, const float* lum_prev, int x, int y,
                      const float4* hit, const float4& albedo, const float4& c) {
    const TpParams& P = A.P;
    const float4 none = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    union { float f; uint32_t u; } flags, node;
    flags.f = hit[0].z;
    node.f = hit[0].y;
    const bool valid = (flags.u & RTU_RAY_HIT) != 0;
    const f3 Pp = mk3(hit[1].x, hit[1].y, hit[1].z), Np = mk3(hit[2].x, hit[2].y, hit[2].z);
    f3 Pm, Nm;
    const bool look = tp_moved_point(in_table, T, Pp, Np, Pm, Nm) && valid && P.lookup != TP_LOOKUP_NONE;
    if (!look || !(tp_finite(c.x) && tp_finite(c.y) && tp_finite(c.z))) return none;
    const bool one_tap = A.same_cam != 0 && (T.flags & RTU_MOTION_STATIC) != 0;
    int qx = x, qy = y;
    if (!one_tap) {
        float fx, fy;
        if (!tp_project(P, Pm, fx, fy)) return none;
        const float rx = floorf(fx + 0.5f), ry = floorf(fy + 0.5f);
        if (!(rx >= 0.0f && rx < (float)P.width && ry >= 0.0f && ry < (float)P.height)) return none;  // (a NaN fails; before the conversion)
        qx = (int)rx;
        qy = (int)ry;
    }
    TpSums S = {mk3(0.0f, 0.0f, 0.0f), 0.0f, 0.0f, 0.0f, 0.0f};
    tp_tap<true>(P, h, qx, qy, 1.0f, Nm, Pm, node.u, P.sigma_plane * hit[0].x, S);
    if (!(S.w > 0.0f)) return none;  // the tap was not ACCEPTED
    const f3 d = dn_demod(albedo);
    const float lc = vr_lum(mk3(c.x / d.x, c.y / d.y, c.z / d.z));
    const float lp = lum_prev[(size_t)qy * (size_t)P.width + (size_t)qx];
    const float var = S.m2 - S.m1 * S.m1;  // (weight 1: S.m1, S.m2 are M_q.x, M_q.y)
    const float noise = one_tap ? 0.0f : 2.0f * (var > 0.0f ? var : 0.0f);
    return make_float4(lc - lp, lc > lp ? lc : lp, noise, 0.0f);
}

// lambda of stratum (sx, sy) out of the gradients `diff` of all strata
RTU_HD float gr_lambda(const GrParams& G, const float4* diff, int sx, int sy) {
    float nsum = 0.0f, dsum = 0.0f, zsum = 0.0f;
    for (int dy = -G.radius; dy <= G.radius; dy++)
        for (int dx = -G.radius; dx <= G.radius; dx++) {
            const int tx = sx + dx, ty = sy + dy;
            if (tx < 0 || ty < 0 || tx >= G.sw || ty >= G.sh) continue;
            const float4 g = diff[(size_t)ty * (size_t)G.sw + (size_t)tx];
            nsum = nsum + g.x;
            dsum = dsum + g.y;
            zsum = zsum + g.z;
        }
    const float x = fabsf(nsum) - G.kappa * sqrtf(zsum);
    const float a = x > 0.0f ? x : 0.0f;  // (a NaN gives 0)
    const float r = a / dsum;
    return (dsum > 0.0f && r == r) ? (r < 1.0f ? r : 1.0f) : 0.0f;
}

// RTU_OK or RTU_ERR_ARG: the rules of RtuGradientDesc (include/rtu_render.h)
int rtu_gradient_check_desc(const RtuGradientDesc* d);

// Every launch function is asynchronous on `stream` and returns a hipError_t as int; pointers 16-byte (float4) or 4-byte aligned and
// descs checked by the caller. S = strata of the image.
// rays[2 * s ..], keys[s], owner[s] for every stratum s: the owner of frame frame_index and its ray and key in the sample `c`
int rtu_launch_gradient_rays(const CamSample& c, uint32_t frame_index, float4* rays, uint32_t* keys, uint32_t* owner, hipStream_t stream);
// lum[p] for every pixel
int rtu_launch_sample_luminance(size_t pixels, const float4* rgbz, const float4* hits, const float4* albedo, float* lum, hipStream_t stream);
// diff[s] and lambda[s] for every stratum: hist_prev (four planes) and lum_prev nullptr with TP_LOOKUP_NONE; an owner outside the image
// gives no gradient
int rtu_launch_temporal_gradient(const GrParams& g, const float4* hits, const float4* albedo, const RtuNodeMotion* d_motion, const float4* hist_prev,
                                 const float* lum_prev, const uint32_t* owner, const float4* rgbt, float4* diff, float* lambda, hipStream_t stream);
// out[p] = lambda[stratum of p] (0 everywhere with lambda == nullptr)
int rtu_launch_lambda_image(int32_t width, int32_t height, const float* lambda, float* out, hipStream_t stream);

#endif
