// rtu_holes.h — the arithmetic of hole rays (include/rtu_render.h "Hole rays"), host + device, and the launch interface of its
// kernels (rtu_holes.hip), called by rtu_capi_temporal.hip:
//   hl_weight   rtu_hole_allocation: 1 for a pixel that has no colour at all and a first hit, 0 for every other. The count, the scan
//               and the cut are st_count / st_cut of rtu_steer.h with max_extra = 1.
//   hl_fold     rtu_hole_fold: the one shaded sample of such a pixel made its history, as the moments form makes a fresh pixel's
// The rays are rtu_extra_sample_rays' (rtu_steer.h). Binary32, one rounding per operation: the translation units that include this
// header are compiled with -ffp-contract=off and IEEE divides, so the host forms and the kernels give the same bits.
#ifndef RTU_HOLES_H_INCLUDED
#define RTU_HOLES_H_INCLUDED

#include "rtu_steer.h"

// ---- 1. allocation ---------------------------------------------------------------------------------------------------------------
// the weight of a pixel whose byte of the hole plane is 1: flags_word the z of the first float4 of its RtuRayHit (the hit record is
// not read for any other pixel)
RTU_HD uint32_t hl_weight(float flags_word) {
    union { float f; uint32_t u; } flags;
    flags.f = flags_word;
    return (flags.u & RTU_RAY_HIT) != 0 ? 1u : 0u;
}

// ---- 3. the fold -----------------------------------------------------------------------------------------------------------------
// A pixel with a hole ray: hole its byte of the hole plane, hit0 the first float4 of its RtuRayHit, c the shaded {r, g, b, t}. Returns
// whether the pixel takes the sample: then E, M and the rgb of rgbz are those of a VALID pixel of rtu_temporal_accumulate_moments that
// found no history (tp_pixel's `fresh`), and the pixel is no hole any more. Else nothing was changed.
RTU_HD bool hl_fold(uint8_t hole, const float4& hit0, const float4& albedo, const float4& c, float4& E, float4& M, float4& rgbz) {
    if (hole != 1 || hl_weight(hit0.z) == 0u) return false;
    if (!(tp_finite(c.x) && tp_finite(c.y) && tp_finite(c.z))) return false;  // the pixel stays a hole: the fill takes it
    const f3 d = dn_demod(albedo);
    const f3 e = mk3(c.x / d.x, c.y / d.y, c.z / d.z);
    const float l = vr_lum(e), l2 = l * l;
    const bool usable = tp_finite(l2);  // else the moments skip the sample (tp_pixel's rule)
    E = make_float4(e.x, e.y, e.z, 1.0f);
    M = usable ? make_float4(l, l2, 0.0f, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    rgbz = make_float4(e.x * d.x, e.y * d.y, e.z * d.z, rgbz.w);
    return true;
}

// RTU_OK or RTU_ERR_ARG: the rules of RtuHoleDesc (include/rtu_render.h)
int rtu_hole_check_desc(const RtuHoleDesc* d);
// the RtuSteerDesc whose count, scan, cut and rays are a hole desc's: its size, budget and frame_index with max_extra = 1
inline RtuSteerDesc hl_steer_desc(const RtuHoleDesc& d) {
    RtuSteerDesc s{};
    s.width = d.width;
    s.height = d.height;
    s.budget = d.budget;
    s.max_extra = 1;
    s.frame_index = d.frame_index;
    return s;
}

// Every launch function is asynchronous on `stream` and returns a hipError_t as int; pointers 16-byte (float4) or 4-byte aligned
// (counts, offsets, total; hole: none) and descs checked by the caller.
// counts[p], offsets[p] and *total of rtu_hole_allocation: k_hole_weight, then the scan of rtu_steer.hip over `scratch`
// (rtu_steer_scratch_words(pixels) words)
int rtu_launch_hole_allocation(const RtuHoleDesc& d, const uint8_t* hole, const float4* hits, uint32_t* counts, uint32_t* offsets, uint32_t* total,
                               uint32_t* scratch, hipStream_t stream);
// the fold: hist four planes (E and M updated in place), rgbz and hole in place; a sample at or beyond n_rays is not read
int rtu_launch_hole_fold(size_t pixels, float4* hist, float4* rgbz, uint8_t* hole, const float4* hits, const float4* albedo, const uint32_t* counts,
                         const uint32_t* offsets, const float4* rgbt, uint32_t n_rays, hipStream_t stream);

#endif
