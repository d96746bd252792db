// render_rays_impl.h — the primary phase of a RAY BATCH (rtu_shade_rays / rtu_shade_rays_device, include/rtu_render.h): the
// root Shade() calls of caller-supplied rays instead of a camera's pixels. Everything behind the roots — k_trace / k_trace2[c] /
// k_consume / k_tail / k_combine — is the launch sequence of render_impl.h, unchanged (launch_all, RTU_LAUNCH_LEVELS): a level-0
// frame carries the index of its ray where a render's carries its pixel, and a.out is the caller's buffer.
//
//   k_ray_roots<STACK, STATS, TEX>   one lane per ray, chunks of 64 rays strided over the grid, the traversal stack in LDS
//                                    (lane-interleaved, as k_primary2 and k_query_closest). Trace() with HitInfo::Init's z replaced
//                                    by tmax (RenderFunctions.cpp:181-212), then the tail of primary_pixel: a miss writes
//                                    environment.SampleEnvironment(dir) — what the reference does for every ray that is not a
//                                    pixel (mtlFunctions.cpp:250, :267, :289) —, a node without material white, a childless
//                                    Shade() call is settled by the lane (shadows_inline + direct_light), anything else is
//                                    appended as a level-0 frame (append_root).
// The fast form walks the 4-wide tree with world-space node bounds: a ray has no pixel, so there are no screen rectangles,
// coverage masks or tile occupancy, and no ray is deferred. STATS walks the reference's tree and counts primary_rays /
// primary_hits as k_primary_counting does. Chunk c appends to shard c % RTU_SHARDS, so ensure_levels(ceil(n / 64)) sizes level 0
// for every root, exactly as for tiles.
// Included by render_rays0.hip .. render_rays3.hip only: the kernels of the render_feat*.hip units are not compiled again.
// RECIPE S (rtu_shade_rays_sampled; render_rays2.hip / render_rays3.hip, feature sets 2|32 and 3|32, RAYD of render_impl.h): the root
// call of ray i has the key keys[i] (ray_keys) where a render's has sample_key(pixel, sample); the ray is given, so the lens and
// pixel-offset draws of primary_pixel are the caller's (rtu_camera_sample_rays). Those two units instantiate the level kernels
// themselves — frame_smp of a level-0 frame reads the key buffer there, which the kernels of render_feat2/3.hip cannot.
#ifndef RTU_RENDER_RAYS_IMPL_H_INCLUDED
#define RTU_RENDER_RAYS_IMPL_H_INCLUDED
// (render_impl.h defines the prelude kernels of a camera's launch sequence, which nothing here launches)
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "render_impl.h"
#include "rtu_query.h"

namespace {

// (three wavefronts per SIMD, as the one-lane-per-ray stage-2 walks it is modelled on: RTU_OCC_WALK)
template <int STACK, bool STATS, int TEX>
__global__ void __launch_bounds__(64) RTU_OCC_WALK k_ray_roots(KernelArgs a, const float4* __restrict__ rays, uint32_t n) {
    __shared__ uint32_t s_stack[STACK * 64];
    const DevScene& s = a.scene;
    const uint32_t lane = threadIdx.x;
    const uint32_t chunks = (n + 63u) / 64u;
    Counters cnt = {};
    Smp smp;
    smp.on = SMPD;  // (recipe S: the sampled feature sets, render_rays2.hip / render_rays3.hip)
    smp.key = 0;
    for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x) {  // whole wavefronts: the tail below votes and appends wave by wave
        const uint32_t i = c * 64u + lane;
        const uint32_t shard = c % RTU_SHARDS;
        float4 ra = make_float4(0, 0, 0, 0), rb = ra;
        if (i < n) { ra = rays[2 * (size_t)i]; rb = rays[2 * (size_t)i + 1]; }
        if (SMPD && i < n) smp.key = ray_keys(a)[i];  // the key of the ray's root Shade() call: the caller's (make_info draws the first refraction normal from it)
        const bool valid = i < n && ray_valid(ra, rb);
        if (i < n && !valid) a.out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // not traced; t == 0 means nothing else (a valid ray has tmax > 0)
        Ray ray;
        ray.p = mk3(ra.x, ra.y, ra.z);
        ray.dir = mk3(rb.x, rb.y, rb.z);  // as given: not renormalised
        Hit h;
        fresh_hit(h, ra.w);
        h.uvw = mk3(0, 0, 0);
        bool want = false;
        int mid = -1;
        if (valid) {
            RTU_CNT(prim);
            bool deferred;
            const bool hit = trace<STACK, STATS, !STATS, false, false, TEXD, false, false, false, true>(s, ray, false, h, s_stack + lane, cnt, deferred);  // FAR: any origin
            if (!hit) {
                const f3 env = (TEXD && s.env.has_map) ? env_sample(s, ray.dir) : ld3(s.environment);
                a.out[i] = make_float4(env.x, env.y, env.z, h.z);  // h.z: still tmax
            } else {
                RTU_CNT(prim_hit);
                mid = as_const(s.nodes)[h.node].material_id;
                if (mid < 0) a.out[i] = make_float4(1.0f, 1.0f, 1.0f, h.z);  // null material => white
                else want = true;
            }
        }
        uint32_t info = 0;
        if (want) info = make_info<TEX>(a, mid, a.frame.max_bounce, h.front, ray.dir, h.p, h.N, h.uvw, smp);
        // A childless Shade() call is settled by the lane that found the hit, as in primary_pixel (rtu_debug_flags 2048 switches
        // this off: results must not change). a.frame.cam_pos is the call's eye. Recipe S, as k_primary_sampled: shadows_inline refuses
        // a call that a soft light reaches — its shadow ray aims at a sample of the light's disk (frame_ray) —, which becomes a frame.
        if (!STATS && !(a.dbg & 2048u) && __any(want && !(info & (RTU_FI_MAIN | RTU_FI_C)))) {
            const bool tryI = want && !(info & (RTU_FI_MAIN | RTU_FI_C));
            uint32_t lit = ~0u;
            bool ok = false;
            if (tryI) ok = shadows_inline<TEX>(a, info, h.p, lit, cnt);
            if (tryI && ok) {
                f3 direct = mk3(0, 0, 0);
                if (info & RTU_FI_SH)
                    direct = direct_light<false, TEX>(a, info, h.p, h.N, h.uvw, ld3(a.frame.cam_pos), direct, [&](uint32_t j) { return ((lit >> j) & 1u) ? 1.0f : 0.0f; });
                a.out[i] = make_float4(direct.x, direct.y, direct.z, h.z);
                want = false;
            }
        }
        append_root<TEX>(a, want, shard, info, h.p, h.N, i, ray.dir, h.z, h.uvw, cnt);
    }
    flush_counters<STATS>(a, cnt);
}

template <int STACK, int TEX>
int launch_ray_roots(const KernelArgs& a, const float4* rays, uint32_t n, bool stats, hipStream_t stream) {
    if (n == 0) return (int)hipSuccess;
    const uint32_t chunks = (n + 63u) / 64u;
    const dim3 grid(chunks < 32768u ? chunks : 32768u);  // (the grid of the one-lane-per-ray walks: launch_all gridN)
    if (stats) hipLaunchKernelGGL((k_ray_roots<STACK, true, TEX>), grid, dim3(64), 0, stream, a, rays, n);
    else hipLaunchKernelGGL((k_ray_roots<STACK, false, TEX>), grid, dim3(64), 0, stream, a, rays, n);
    return (int)hipGetLastError();
}

template <int TEX>
int launch_ray_roots_stack(const KernelArgs& a, const float4* rays, uint32_t n, uint32_t bvh_stack_needed, bool stats, hipStream_t stream) {
    if (bvh_stack_needed <= 16) return launch_ray_roots<16, TEX>(a, rays, n, stats, stream);
    if (bvh_stack_needed <= 24) return launch_ray_roots<24, TEX>(a, rays, n, stats, stream);
    if (bvh_stack_needed <= 32) return launch_ray_roots<32, TEX>(a, rays, n, stats, stream);
    return launch_ray_roots<RTU_MAX_BVH_STACK, TEX>(a, rays, n, stats, stream);
}

}  // namespace

#endif
