// rtu_variance.h — the arithmetic of the variance-guided preview filter (include/rtu_render.h "Variance-guided filtering"), host +
// device, and the launch interface of its kernels (rtu_variance.hip), called by rtu_capi_temporal.hip:
//   vr_variance_pixel   rtu_variance: the variance of the accumulated mean out of E.n and M
//   vd_*                rtu_denoise_variance: the a-trous passes of rtu_denoise.h with a per-pixel colour edge-stop
// The moments themselves are accumulated by tp_pixel<true, true> of rtu_temporal.h (a MOMENTS HISTORY, vr_lum).
// No transcendental function: the translation units that include this header are compiled with -ffp-contract=off and IEEE divides
// and square roots, every operation below rounds once, so the host forms and the kernels give the same bits.
#ifndef RTU_VARIANCE_H_INCLUDED
#define RTU_VARIANCE_H_INCLUDED

#include "rtu_temporal.h"

#define VR_EPS 1e-8f  // added to sigma_lum^2 g3(v): a pixel without variance still accepts taps of its own luminance

// ---- 1. the variance of the accumulated mean -------------------------------------------------------------------------------------
struct VrParams {
    int32_t width, height, nlog2;
    float   min_history, sigma_plane;
};

inline VrParams vr_setup(const RtuVarianceDesc& d) {
    VrParams V{};
    V.width = d.width;
    V.height = d.height;
    V.nlog2 = d.normal_log2_power;
    V.min_history = (float)d.min_history;
    V.sigma_plane = d.sigma_plane;
    return V;
}

// the guide weight of a tap: t wp of dn_tap, the plane term with p's reciprocal rp = 1 / (sigma_plane t_p)
RTU_HD float vr_guide_weight(const f3& Np, const f3& Pp, float rp, const f3& Nq, const f3& Pq, int nlog2) {
    const float dot = dot3(Np, Nq);
    float t = dot > 0.0f ? dot : 0.0f;
    for (int j = 0; j < nlog2; j++) t = t * t;
    const float x = dot3(Np, Pq - Pp) * rp;
    const float wp = 1.0f / (1.0f + x * x);
    return t * wp;
}

// Pixel (x, y): hE, hM the first and the fourth plane of a moments history, hits three float4 per pixel (RtuRayHit).
RTU_HD float vr_variance_pixel(const VrParams& V, const float4* hE, const float4* hM, const float4* hits, int x, int y) {
    const size_t p = (size_t)y * (size_t)V.width + (size_t)x;
    const float4 hit0 = hits[3 * p], Ep = hE[p], Mp = hM[p];
    union { float f; uint32_t u; } flags;
    flags.f = hit0.z;
    const float n = Ep.w;
    const bool live = (flags.u & RTU_RAY_HIT) != 0 && n > 0.0f;
    const float dt = Mp.y - Mp.x * Mp.x;
    const float vt = dt > 0.0f ? dt : 0.0f;  // (a NaN gives 0)
    float var = vt;
    if (live && n < V.min_history) {  // a short history: the moments of the neighbourhood that shows the same surface
        const float4 h1 = hits[3 * p + 1], h2 = hits[3 * p + 2];
        const f3 Pp = mk3(h1.x, h1.y, h1.z), Np = mk3(h2.x, h2.y, h2.z);
        const float rp = 1.0f / (V.sigma_plane * hit0.x);
        float s1 = 0.0f, s2 = 0.0f, ws = 0.0f;
        for (int dy = -3; dy <= 3; dy++) {
            const int qy = y + dy;
            if (qy < 0 || qy >= V.height) continue;
            for (int dx = -3; dx <= 3; dx++) {
                const int qx = x + dx;
                if (qx < 0 || qx >= V.width) continue;
                const size_t q = (size_t)qy * (size_t)V.width + (size_t)qx;
                union { float f; uint32_t u; } fq;
                fq.f = hits[3 * q].z;
                if ((fq.u & RTU_RAY_HIT) == 0 || !(hE[q].w > 0.0f)) continue;
                const float4 q1 = hits[3 * q + 1], q2 = hits[3 * q + 2], Mq = hM[q];
                const float w = vr_guide_weight(Np, Pp, rp, mk3(q2.x, q2.y, q2.z), mk3(q1.x, q1.y, q1.z), V.nlog2);
                s1 = s1 + Mq.x * w;
                s2 = s2 + Mq.y * w;
                ws = ws + w;
            }
        }
        float vs = 0.0f;
        if (ws > 0.0f) {
            const float a1 = s1 / ws, a2 = s2 / ws;
            const float ds = a2 - a1 * a1;
            vs = ds > 0.0f ? ds : 0.0f;
        }
        var = (vs > vt ? vs : vt) * (V.min_history / n);
    }
    return live ? var / n : 0.0f;
}

// ---- 2. the filter ---------------------------------------------------------------------------------------------------------------
// Four planes of one float4 per pixel, as rtu_denoise.h:
//   gN = {N.xyz, valid ? 1 : 0}      gP = {p.xyz, 1 / (sigma_plane * t)}      e = {demodulated rgb, v}, two of them, ping-pong
RTU_HD void vd_prepare(const float4& rgbz, const float4* hit, const float4& albedo, float v, float sigma_plane, float4& gN, float4& gP, float4& e) {
    union { float f; uint32_t u; } flags;
    flags.f = hit[0].z;
    const bool valid = (flags.u & RTU_RAY_HIT) != 0;
    const f3 d = dn_demod(albedo);
    gN = make_float4(hit[2].x, hit[2].y, hit[2].z, valid ? 1.0f : 0.0f);
    gP = make_float4(hit[1].x, hit[1].y, hit[1].z, 1.0f / (sigma_plane * hit[0].x));
    e = make_float4(rgbz.x / d.x, rgbz.y / d.y, rgbz.z / d.z, v);
}

// One pass at pixel (x, y), valid. sl2 = sigma_lum * sigma_lum. Returns the new {e_p, v_p}.
// Written for the device: every tap is loaded — from a clamped address where it lies outside the image — and a tap that is skipped
// leaves the sums as they are by a select, so the loads of a row of taps do not wait for one another's tests.
RTU_HD float4 vd_pass_pixel(const float4* gN, const float4* gP, const float4* e, int width, int height, int x, int y, int step, float sl2, int nlog2) {
    const size_t p = (size_t)y * (size_t)width + (size_t)x;
    const float4 gNp = gN[p], gPp = gP[p], ep = e[p];
    const f3 Np = mk3(gNp.x, gNp.y, gNp.z), Pp = mk3(gPp.x, gPp.y, gPp.z);
    // g3: the 3 x 3 binomial of v over the valid neighbours at distance 1, whatever the step (p itself is one of them)
    float g = 0.0f, ks = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        const bool iny = qy >= 0 && qy < height;
        const size_t row = (size_t)(iny ? qy : y) * (size_t)width;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            const bool inx = qx >= 0 && qx < width;
            const size_t q = row + (size_t)(inx ? qx : x);
            const bool use = iny && inx && gN[q].w != 0.0f;
            const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
            g = use ? g + e[q].w * k : g;
            ks = use ? ks + k : ks;
        }
    }
    g = g / ks;
    const float rp = 1.0f / (sl2 * g + VR_EPS);
    const float lp = vr_lum(mk3(ep.x, ep.y, ep.z));
    f3 acc = mk3(0, 0, 0);
    float vacc = 0.0f, wsum = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {  // (int suffices: x, y < 65536 and step <= 128 by rtu_variance_check_desc, |dy * step| <= 256)
        const int qy = y + dy * step;
        const bool iny = qy >= 0 && qy < height;
        const size_t row = (size_t)(iny ? qy : y) * (size_t)width;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * step;
            const bool inx = qx >= 0 && qx < width;
            const size_t q = row + (size_t)(inx ? qx : x);
            const float4 gNq = gN[q], gPq = gP[q], eq = e[q];
            const bool use = iny && inx && gNq.w != 0.0f;
            const f3 cq = mk3(eq.x, eq.y, eq.z);
            const float h = dn_k(dy + 2) * dn_k(dx + 2);
            const float tw = vr_guide_weight(Np, Pp, gPp.w, mk3(gNq.x, gNq.y, gNq.z), mk3(gPq.x, gPq.y, gPq.z), nlog2);
            const float dl = vr_lum(cq) - lp;
            const float wc = 1.0f / (1.0f + (dl * dl) * rp);
            const float w = (h * tw) * wc;
            acc.x = use ? acc.x + cq.x * w : acc.x;
            acc.y = use ? acc.y + cq.y * w : acc.y;
            acc.z = use ? acc.z + cq.z * w : acc.z;
            vacc = use ? vacc + eq.w * (w * w) : vacc;
            wsum = use ? wsum + w : wsum;
        }
    }
    if (wsum > 0.0f) {
        const float ws2 = wsum * wsum;
        return make_float4(acc.x / wsum, acc.y / wsum, acc.z / wsum, ws2 > 0.0f ? vacc / ws2 : ep.w);
    }
    return ep;
}

// RTU_OK or RTU_ERR_ARG: the rules of RtuVarianceDesc (include/rtu_render.h)
int rtu_variance_check_desc(const RtuVarianceDesc* d);

// v[i] = the variance of pixel i: hist four planes of width * height float4, hits width * height RtuRayHit
int rtu_launch_variance(const VrParams& V, const float4* hist, const float4* hits, float* v, hipStream_t stream);
// The filter on the device: as rtu_launch_denoise, v width * height floats; planes four arrays of width * height float4.
int rtu_launch_denoise_variance(const RtuVarianceDesc& desc, const float4* rgbz_in, const float4* hits, const float4* albedo, const float* v,
                                float4* rgbz_out, float4* planes, hipStream_t stream);

#endif
