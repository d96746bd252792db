// rtu_query.h — launch interface of the ray-query kernels (rtu_query.hip), called by rtu_capi.hip.
#ifndef RTU_QUERY_H_INCLUDED
#define RTU_QUERY_H_INCLUDED

#include "rtu_device.h"

// rays: n RtuRay (two float4 each), hits: n RtuRayHit (three float4 each), occluded: n bytes. Both pointers 16-byte aligned
// (checked by the caller). n == 0 launches nothing. Returns a hipError_t as int. Asynchronous on `stream`.
int rtu_launch_query_closest(const DevScene& s, const float4* rays, float4* hits, unsigned long long n, bool reference_walk, hipStream_t stream);
int rtu_launch_query_any(const DevScene& s, const float4* rays, uint8_t* occluded, unsigned long long n, bool reference_walk, hipStream_t stream);

#endif
