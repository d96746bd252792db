// rtu_query.hip — ray queries (rtu_trace_rays / rtu_occluded_rays, include/rtu_render.h): the scene walk of the renderer,
// trace<> of rtu_intersect.h, fed from a buffer of caller-supplied rays instead of a camera.
//
//   k_query_closest<REFWALK>   Trace() of every ray (RenderFunctions.cpp:181-212): one RtuRayHit per ray
//   k_query_any<REFWALK>       ShadowTrace() of every ray and GenLight::Shadow's conclusion `hit && z > 0`
//                              (RenderFunctions.cpp:214-240, lightFunctions.cpp:27-37): one byte per ray
//
// One ray per lane, 64-thread workgroups, the traversal stack in LDS (RTU_MAX_BVH_STACK entries per lane, lane-interleaved:
// 12 KB per workgroup, 13 workgroups per CU), a grid-stride loop over chunks of 64 rays like the stage-2 walks of
// render_impl.h (k_primary2 / k_trace2). REFWALK = false is the fast variant as those kernels instantiate it — the 4-wide SAH
// tree with culling, node-level bounds in world space, exact ties and stack overflows finished on the reference's tree;
// REFWALK = true is the counting variant's walk (the reference's own tree, no culling) with its counters thrown away. Both
// read the DevScene the renders read, so rtu_debug_walk_stack_limit / rtu_debug_node_bounds apply.
//
// A ray is validated BEFORE the walk (ray_valid): trace<> and its conservative bounds were argued and are tested for the
// renderer's own rays — finite, unit length. Anything else is answered RTU_RAY_INVALID without being traced.
// Arbitrary rays carry no list-length hint and no coherence promise: there is no LDS tree staging, no cooperative form
// and no occluder list (lslot = -1).
#include "rtu_intersect.h"
#include "rtu_query.h"

namespace {

// three wavefronts per SIMD, as the stage-2 walks (RTU_OCC_WALK): the 12 KB LDS stack allows 13 workgroups per CU
#define RTU_OCC_QUERY __attribute__((amdgpu_waves_per_eu(3, 3)))

// (ray_valid: rtu_query.h)
template <bool REFWALK, bool SHADOW>
__device__ __forceinline__ bool query_trace(const DevScene& s, const float4& a, const float4& b, Hit& h, uint32_t* stk) {
    Ray ray;
    ray.p = mk3(a.x, a.y, a.z);
    ray.dir = mk3(b.x, b.y, b.z);  // as given: not renormalised
    fresh_hit(h, a.w);
    Counters cnt = {};
    bool deferred;
    if (REFWALK) return trace<RTU_MAX_BVH_STACK, true, false, false>(s, ray, SHADOW, h, stk, cnt, deferred);
    return trace<RTU_MAX_BVH_STACK, false, true, false, false, false, false, false, false, true>(s, ray, SHADOW, h, stk, cnt, deferred);  // FAR: any origin
}

template <bool REFWALK>
__global__ void __launch_bounds__(64) RTU_OCC_QUERY k_query_closest(DevScene s, const float4* __restrict__ rays, float4* __restrict__ hits,
                                                                    unsigned long long n) {
    __shared__ uint32_t s_stack[RTU_MAX_BVH_STACK * 64];
    const uint32_t lane = threadIdx.x;
    const unsigned long long chunks = (n + 63ull) / 64ull;
    for (unsigned long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const unsigned long long i = c * 64ull + lane;
        if (i >= n) continue;
        const float4 a = rays[2 * i], b = rays[2 * i + 1];
        Hit h;
        fresh_hit(h, a.w);
        uint32_t flags = RTU_RAY_INVALID;
        int material = -1;
        if (ray_valid(a, b)) {
            const bool hit = query_trace<REFWALK, false>(s, a, b, h, s_stack + lane);
            flags = (hit ? RTU_RAY_HIT : 0u) | (hit && h.front ? RTU_RAY_FRONT : 0u);
            if (hit) material = s.nodes[h.node].material_id;  // per-lane node: an ordinary load
            else { h.node = -1; h.p = mk3(0, 0, 0); h.N = mk3(0, 0, 0); }
        }
        hits[3 * i] = make_float4(h.z, __int_as_float(h.node), __uint_as_float(flags), __int_as_float(material));
        hits[3 * i + 1] = make_float4(h.p.x, h.p.y, h.p.z, 0.0f);
        hits[3 * i + 2] = make_float4(h.N.x, h.N.y, h.N.z, 0.0f);
    }
}

template <bool REFWALK>
__global__ void __launch_bounds__(64) RTU_OCC_QUERY k_query_any(DevScene s, const float4* __restrict__ rays, uint8_t* __restrict__ occluded,
                                                                unsigned long long n) {
    __shared__ uint32_t s_stack[RTU_MAX_BVH_STACK * 64];
    const uint32_t lane = threadIdx.x;
    const unsigned long long chunks = (n + 63ull) / 64ull;
    for (unsigned long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const unsigned long long i = c * 64ull + lane;
        if (i >= n) continue;
        const float4 a = rays[2 * i], b = rays[2 * i + 1];
        bool occ = false;
        if (ray_valid(a, b)) {
            Hit h;
            const bool hit = query_trace<REFWALK, true>(s, a, b, h, s_stack + lane);
            occ = hit && h.z > 0.0f;  // GenLight::Shadow, lightFunctions.cpp:33
        }
        occluded[i] = occ ? (uint8_t)1 : (uint8_t)0;
    }
}

// enough workgroups to fill every CU several times over (13 fit per CU); longer batches stride
uint32_t query_grid(unsigned long long n) {
    const unsigned long long chunks = (n + 63ull) / 64ull;
    return (uint32_t)(chunks < 8192ull ? chunks : 8192ull);
}

}  // namespace

int rtu_launch_query_closest(const DevScene& s, const float4* rays, float4* hits, unsigned long long n, bool reference_walk, hipStream_t stream) {
    if (n == 0) return (int)hipSuccess;
    if (reference_walk) hipLaunchKernelGGL(k_query_closest<true>, dim3(query_grid(n)), dim3(64), 0, stream, s, rays, hits, n);
    else hipLaunchKernelGGL(k_query_closest<false>, dim3(query_grid(n)), dim3(64), 0, stream, s, rays, hits, n);
    return (int)hipGetLastError();
}

int rtu_launch_query_any(const DevScene& s, const float4* rays, uint8_t* occluded, unsigned long long n, bool reference_walk, hipStream_t stream) {
    if (n == 0) return (int)hipSuccess;
    if (reference_walk) hipLaunchKernelGGL(k_query_any<true>, dim3(query_grid(n)), dim3(64), 0, stream, s, rays, occluded, n);
    else hipLaunchKernelGGL(k_query_any<false>, dim3(query_grid(n)), dim3(64), 0, stream, s, rays, occluded, n);
    return (int)hipGetLastError();
}
