// rtu_denoise.h — the arithmetic of the denoising filter (rtu_denoise / rtu_denoise_device, include/rtu_render.h), host + device, and
// the launch interface of its kernels (rtu_denoise.hip), called by rtu_capi.hip.
//
// An edge-avoiding a-trous wavelet filter on albedo-demodulated colour, guided by the first-hit normal, position and depth of
// rtu_ray_features / rtu_frame_features. No transcendental function: the translation units that include this header are compiled
// with -ffp-contract=off and IEEE divides, every operation below rounds once, so the host form and the kernels give the same bits.
//
// Both forms work on four PLANES of one float4 per pixel, made by dn_prepare from the caller's three arrays:
//   gN = {N.xyz, valid ? 1 : 0}      gP = {p.xyz, sigma_plane * t}      e = {demodulated rgb, 0}, two of them, ping-pong
#ifndef RTU_DENOISE_H_INCLUDED
#define RTU_DENOISE_H_INCLUDED

#include "rtu_render.h"
#include "rtu_vec.h"

#include <stddef.h>

// d = a > 0.01f ? a : 1.0f per channel: what the colour is divided by going in and multiplied by coming out
RTU_HD f3 dn_demod(const float4& albedo) {
    return mk3(albedo.x > 0.01f ? albedo.x : 1.0f, albedo.y > 0.01f ? albedo.y : 1.0f, albedo.z > 0.01f ? albedo.z : 1.0f);
}

// the planes of one pixel. hit: the three float4 of its RtuRayHit {t, node, flags, material} {p, -} {N, -}
RTU_HD void dn_prepare(const float4& rgbz, const float4* hit, const float4& albedo, float sigma_plane, float4& gN, float4& gP, float4& e) {
    union { float f; uint32_t u; } flags;
    flags.f = hit[0].z;
    const bool valid = (flags.u & RTU_RAY_HIT) != 0;
    const f3 d = dn_demod(albedo);
    gN = make_float4(hit[2].x, hit[2].y, hit[2].z, valid ? 1.0f : 0.0f);
    gP = make_float4(hit[1].x, hit[1].y, hit[1].z, sigma_plane * hit[0].x);
    e = make_float4(rgbz.x / d.x, rgbz.y / d.y, rgbz.z / d.z, 0.0f);
}

// k = {1/16, 1/4, 3/8, 1/4, 1/16}: the B3 spline; every product of two of them is exact
RTU_HD float dn_k(int i) { return (i == 0 || i == 4) ? 0.0625f : (i == 2 ? 0.375f : 0.25f); }

// One tap q of pixel p: its weight w = ((h t) wp) wc, added to wsum, and e_q w, added to acc.
//   t   max(Np . Nq, 0), a NaN giving 0, squared nlog2 times          (the normals agree)
//   wp  1 / (1 + x x), x = (Np . (Pq - Pp)) / (sigma_plane t_p)       (q lies in p's tangent plane, on the scale of p's depth)
//   wc  1 / (1 + |e_q - e_p|^2 / sc2)                                 (the colours agree, on this pass's scale)
RTU_HD void dn_tap(float h, const float4& gNp, const float4& gPp, const float4& ep, const float4& gNq, const float4& gPq, const float4& eq, float sc2,
                   int nlog2, f3& acc, float& wsum) {
    const f3 Np = mk3(gNp.x, gNp.y, gNp.z), Nq = mk3(gNq.x, gNq.y, gNq.z);
    const float dot = dot3(Np, Nq);
    float t = dot > 0.0f ? dot : 0.0f;
    for (int j = 0; j < nlog2; j++) t = t * t;
    const f3 D = mk3(gPq.x, gPq.y, gPq.z) - mk3(gPp.x, gPp.y, gPp.z);
    const float dd = dot3(Np, D);
    const float x = dd / gPp.w;
    const float wp = 1.0f / (1.0f + x * x);
    const f3 dl = mk3(eq.x, eq.y, eq.z) - mk3(ep.x, ep.y, ep.z);
    const float dc = dot3(dl, dl);
    const float wc = 1.0f / (1.0f + dc / sc2);
    const float w = ((h * t) * wp) * wc;
    acc = acc + mk3(eq.x, eq.y, eq.z) * w;
    wsum = wsum + w;
}

// One pass at pixel (x, y), valid: the 25 taps p + step * (dx, dy), dy outer, dx inner, skipping those outside the image or not
// valid; every tap reads the previous pass's e. Returns the new e_p (e_p itself where no tap has weight).
RTU_HD float4 dn_pass_pixel(const float4* gN, const float4* gP, const float4* e, int width, int height, int x, int y, int step, float sc2, int nlog2) {
    const size_t p = (size_t)y * (size_t)width + (size_t)x;
    const float4 gNp = gN[p], gPp = gP[p], ep = e[p];
    f3 acc = mk3(0, 0, 0);
    float wsum = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const long long qy = (long long)y + (long long)dy * step;
        if (qy < 0 || qy >= height) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const long long qx = (long long)x + (long long)dx * step;
            if (qx < 0 || qx >= width) continue;
            const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
            const float4 gNq = gN[q];
            if (gNq.w == 0.0f) continue;
            dn_tap(dn_k(dy + 2) * dn_k(dx + 2), gNp, gPp, ep, gNq, gP[q], e[q], sc2, nlog2, acc, wsum);
        }
    }
    if (wsum > 0.0f) return make_float4(acc.x / wsum, acc.y / wsum, acc.z / wsum, 0.0f);
    return ep;
}

// the output pixel: e * d where valid, else the input rgb as it is; the input z always
RTU_HD float4 dn_output(const float4& rgbz, const float4& albedo, bool valid, const float4& e) {
    if (!valid) return rgbz;
    const f3 d = dn_demod(albedo);
    return make_float4(e.x * d.x, e.y * d.y, e.z * d.z, rgbz.w);
}

// sc2 of pass i: sc = sigma_color * 2^-i (an exact scaling), sc2 = sc * sc
inline float dn_sc2(float sigma_color, int pass) {
    const float sc = sigma_color * (1.0f / (float)(1u << pass));
    return sc * sc;
}

// RTU_OK or RTU_ERR_ARG: the rules of RtuDenoiseDesc (include/rtu_render.h)
int rtu_denoise_check_desc(const RtuDenoiseDesc* d);

// The filter on the device: rgbz_in, albedo, rgbz_out [width * height] float4, hits [width * height] RtuRayHit; planes: four
// arrays of width * height float4 (gN, gP, e0, e1). rgbz_out == rgbz_in is allowed. Pointers 16-byte aligned and desc checked by
// the caller. Returns a hipError_t as int. Asynchronous on `stream`.
int rtu_launch_denoise(const RtuDenoiseDesc& desc, const float4* rgbz_in, const float4* hits, const float4* albedo, float4* rgbz_out,
                       float4* planes, hipStream_t stream);

#endif
