// rtu_steer.h — the arithmetic of steered sampling (include/rtu_render.h "Steered sampling"), host + device, and the launch interface
// of its kernels (rtu_steer.hip), called by rtu_capi_temporal.hip:
//   st_weight / st_count / st_cut   rtu_sample_allocation: a budget of extra rays spread by the variance of the accumulated mean
//   st_extra_ray                    rtu_extra_sample_rays: extra sample j of a pixel, through camera_sample_ray of rtu_camrays.h
//   st_refine_pixel                 rtu_temporal_refine: the extra samples of a pixel folded into its E, M and image
// The weights are integers and their sum is exact, so the allocation does not depend on the order in which anything is added. The
// floating-point expressions round once per operation: the translation units that include this header are compiled with
// -ffp-contract=off and IEEE divides, so the host forms and the kernels give the same bits.
#ifndef RTU_STEER_H_INCLUDED
#define RTU_STEER_H_INCLUDED

#include "rtu_camrays.h"
#include "rtu_temporal.h"

#define ST_REL_EPS   1.0f         // added to m1^2: the absolute variance of the mean for a dark pixel, the relative one for a bright one
#define ST_SCALE     16777216.0f  // a variance of 2^-24 weighs 1
#define ST_WEIGHT_MAX 1048576u    // ... and 2^-4 or more weigh 2^20
#define ST_MAX_EXTRA 15

// ---- 1. allocation ---------------------------------------------------------------------------------------------------------------
// the weight of a pixel: hit0 the first float4 of its RtuRayHit, Ep and Mp its pixels of the planes E and M, v its variance
RTU_HD uint32_t st_weight(const float4& hit0, const float4& Ep, const float4& Mp, float v) {
    union { float f; uint32_t u; } flags;
    flags.f = hit0.z;
    const bool live = (flags.u & RTU_RAY_HIT) != 0 && Ep.w > 0.0f;
    const float x = (v / (Mp.x * Mp.x + ST_REL_EPS)) * ST_SCALE;
    if (!live || !(x > 0.0f)) return 0u;  // (a NaN fails)
    return x >= (float)ST_WEIGHT_MAX ? ST_WEIGHT_MAX : (uint32_t)x;
}

// the count of pixel p before the cut: its share of the budget, rounded by a dither of the pixel and the frame, at most max_extra
RTU_HD uint32_t st_count(uint32_t p, uint32_t w, unsigned long long wsum, uint32_t budget, uint32_t max_extra, uint32_t frame_index) {
    if (wsum == 0ull) return 0u;
    const unsigned long long h = (unsigned long long)(cs_mix32(p + 0x9e3779b9u * (frame_index + 1u)) >> 16);
    const unsigned long long c = ((unsigned long long)budget * (unsigned long long)w + ((h * wsum) >> 16)) / wsum;
    return c < (unsigned long long)max_extra ? (uint32_t)c : max_extra;
}

// the cut at the budget in pixel order: c the count and o the exclusive scan of the counts before the cut
RTU_HD void st_cut(uint32_t c, uint32_t o, uint32_t budget, uint32_t& c_out, uint32_t& o_out) {
    const uint32_t start = o < budget ? o : budget;
    const uint32_t room = budget - start;
    c_out = c < room ? c : room;
    o_out = start;
}

// ---- 2. the extra rays -----------------------------------------------------------------------------------------------------------
// The camera of the frame with samples = S (1 + E), and the pixel offsets of its samples sample0 + j, j < E (made on the host:
// launch()'s expressions, as CamSample's). c.ox, c.oy and c.sample are not read.
struct StRays {
    CamSample c;
    float     ox[ST_MAX_EXTRA], oy[ST_MAX_EXTRA];
    uint32_t  sample0;
};

// extra sample j of pixel (x, y): the ray and key of rtu_camera_sample_rays(frame with samples = S (1 + E), sample0 + j)
template <class SinCos>
RTU_HD void st_extra_ray(const CamSample& base, float ox, float oy, uint32_t sample, int x, int y, SinCos sc, f3& org, f3& dir, uint32_t& key) {
    CamSample c = base;
    c.ox = ox;
    c.oy = oy;
    c.sample = sample;
    camera_sample_ray(c, x, y, sc, org, dir, key);
}

// ---- 3. the fold -----------------------------------------------------------------------------------------------------------------
// Pixel p with count samples, rgbt their {r, g, b, t} (the first of them): E, M and rgbz of the pixel are updated. Returns whether
// the pixel takes samples at all (else nothing was changed).
RTU_HD bool st_refine_pixel(float max_history, const float4& hit0, const float4& albedo, uint32_t count, const float4* rgbt, float4& E, float4& M,
                            float4& rgbz) {
    union { float f; uint32_t u; } flags;
    flags.f = hit0.z;
    if ((flags.u & RTU_RAY_HIT) == 0 || !(E.w > 0.0f) || count == 0u) return false;
    const f3 d = dn_demod(albedo);
    f3 e = mk3(E.x, E.y, E.z);
    float n = E.w, m1 = M.x, m2 = M.y;
    for (uint32_t j = 0; j < count; j++) {
        const float4 c = rgbt[j];
        if (!(tp_finite(c.x) && tp_finite(c.y) && tp_finite(c.z))) continue;  // the sample is not accumulated
        const f3 e_cur = mk3(c.x / d.x, c.y / d.y, c.z / d.z);
        n = smin(n + 1.0f, max_history);
        const float a = 1.0f / n;
        e = e + (e_cur - e) * a;
        const float l = vr_lum(e_cur), l2 = l * l;
        if (tp_finite(l2)) {  // else the moments skip the sample (tp_pixel's rule)
            m1 = m1 + (l - m1) * a;
            m2 = m2 + (l2 - m2) * a;
        }
    }
    E = make_float4(e.x, e.y, e.z, n);
    M = make_float4(m1, m2, M.z, M.w);
    rgbz = make_float4(e.x * d.x, e.y * d.y, e.z * d.z, rgbz.w);
    return true;
}

// RTU_OK or RTU_ERR_ARG: the rules of RtuSteerDesc (include/rtu_render.h)
int rtu_steer_check_desc(const RtuSteerDesc* d);
// words of scratch the allocation needs for `pixels` pixels (16-byte aligned)
size_t rtu_steer_scratch_words(size_t pixels);

// where the allocation keeps what in its scratch of rtu_steer_scratch_words(pixels) words: Wsum (64 bits, 8-byte aligned), the total
// before the cut, one weight per pixel (16-byte aligned, padded to whole groups of four) and one sum per tile of 1024 pixels
struct StScratch {
    unsigned long long* wsum;
    uint32_t *raw_total, *w, *sums;
};
inline StScratch st_scratch(uint32_t* scratch, size_t pixels) {
    return StScratch{reinterpret_cast<unsigned long long*>(scratch), scratch + 2, scratch + 4, scratch + 4 + 4 * ((pixels + 3) / 4)};
}

// counts[p], offsets[p] and *total of rtu_sample_allocation for the width * height pixels of `d`: hist four planes, hits RtuRayHit, v
// floats. Asynchronous on `stream`; every launch function returns a hipError_t as int.
int rtu_launch_sample_allocation(const RtuSteerDesc& d, const float4* hist, const float4* hits, const float* v, uint32_t* counts, uint32_t* offsets,
                                 uint32_t* total, uint32_t* scratch, hipStream_t stream);
// The allocation behind its weights (k_steer_counts, k_steer_sums, k_steer_finish): s.w and *s.wsum are written on `stream` by the
// caller's own weight kernel, after a hipMemsetAsync of the first 16 bytes of the scratch. Of `d` the size, budget, max_extra and
// frame_index are used. "Hole rays" (rtu_holes.hip) allocates through this with weights of its own.
int rtu_launch_allocation_scan(const RtuSteerDesc& d, const StScratch& s, uint32_t* counts, uint32_t* offsets, uint32_t* total, hipStream_t stream);
// rays[2 * (o_p + j) ..], keys[o_p + j], owner[o_p + j] for j < c_p; a ray at or beyond `capacity` is not written
int rtu_launch_extra_sample_rays(const StRays& r, uint32_t max_extra, const uint32_t* counts, const uint32_t* offsets, float4* rays, uint32_t* keys,
                                 uint32_t* owner, uint32_t capacity, hipStream_t stream);
// the fold: hist four planes, updated in place (E and M), rgbz in place; a sample at or beyond n_rays is not read
int rtu_launch_temporal_refine(size_t pixels, float max_history, float4* hist, const float4* hits, const float4* albedo, const uint32_t* counts,
                               const uint32_t* offsets, const float4* rgbt, uint32_t n_rays, float4* rgbz, hipStream_t stream);

#endif
