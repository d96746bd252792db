// rtu_query.h — launch interface of the ray-query kernels (rtu_query.hip), called by rtu_capi.hip.
#ifndef RTU_QUERY_H_INCLUDED
#define RTU_QUERY_H_INCLUDED

#include "rtu_device.h"
#include "rtu_vec.h"

// rtu_render.h "Invalid rays": every component finite, tmax > 0, |dot(dir, dir) - 1| <= 2e-3 (binary32, dot3's order). a = {org, tmax},
// b = {dir, reserved}: the two float4 of an RtuRay. Shared by the ray queries (rtu_query.hip) and the ray batches (render_rays_impl.h).
__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ bool ray_valid(const float4& a, const float4& b) {
    const bool fin = finite_bits(a.x) && finite_bits(a.y) && finite_bits(a.z) && finite_bits(a.w) && finite_bits(b.x) && finite_bits(b.y) &&
                     finite_bits(b.z);
    const float dd = dot3(mk3(b.x, b.y, b.z), mk3(b.x, b.y, b.z));
    return fin && a.w > 0.0f && !(fabsf(dd - 1.0f) > 2e-3f);
}

// rays: n RtuRay (two float4 each), hits: n RtuRayHit (three float4 each), occluded: n bytes. Both pointers 16-byte aligned
// (checked by the caller). n == 0 launches nothing. Returns a hipError_t as int. Asynchronous on `stream`.
int rtu_launch_query_closest(const DevScene& s, const float4* rays, float4* hits, unsigned long long n, bool reference_walk, hipStream_t stream);
int rtu_launch_query_any(const DevScene& s, const float4* rays, uint8_t* occluded, unsigned long long n, bool reference_walk, hipStream_t stream);

#endif
