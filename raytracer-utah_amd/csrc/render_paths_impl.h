// render_paths_impl.h — the front of a PATH-TRACED RAY BATCH (rtu_shade_rays_paths / rtu_shade_rays_paths_device, include/rtu_render.h):
// recipe P along caller-supplied rays. A chain of recipe P is a primary hit and the four gather rays behind it
// (RenderFunctions.cpp:549-590); the frame path traces it inside k_primary_sampled / k_primary2[c], which find their work through
// tiles, pixels and shards (primary_pixel, render_impl.h). Here the chain index is the ray index:
//
//   k_path_roots<STACK, STATS, TEX>  k_ray_roots (render_rays_impl.h) with the recipe-P tail of primary_pixel: one lane per ray, chunks
//                                    of 64 strided over the grid, the traversal stack in LDS. A hit does not become a frame: it
//                                    becomes the depth-0 record of chain i in gi_h — {p, z} {N, hit | front << 1 | (mtl + 1) << 2}
//                                    {dir, keys[i]} {uvw, -} —, keys[i] being the key of the ray's root call. A miss writes
//                                    environment.SampleEnvironment(dir) and t = tmax to a.out[i] itself, an invalid ray sixteen zero
//                                    bytes, a node without material white; all three leave a record whose hit bit is clear, which is
//                                    "no hit" to every deeper depth, to k_gi_roots and to k_gi_final.
//   k_path_step<STACK, STATS, TEX>   depth k = a.gi_depth = 1 .. 4 of every chain: the `a.gi_depth > 0` block of primary_pixel fed by
//                                    the chain index — read depth k - 1; no hit there: no hit here; otherwise SampleHemiSphereCosine
//                                    from the hit's key (purposes 0x40000 / 0x40001), the gather ray's hit continues with
//                                    child_key(key, RTU_SLOT_GATHER), Trace(), write depth k. One lane per chain, no second stage:
//                                    a gather ray starts anywhere in the scene, so its wavefront has no screen coherence to lose.
// What follows — k_gi_roots at every depth from the deepest up, the recursion levels behind it, k_gi_final — is the frame path's own
// launch sequence in the units render_feat10.hip / render_feat11.hip AS COMPILED (rtu_launch_frame, RTU_LAUNCH_SHADE): k_gi_roots
// addresses gi_h / gi_res by chain, a recipe-P level-0 frame carries its key in fb.w (frame_smp) and its chain in fc.w, the level
// kernels write gi_res[chain], k_gi_final adds two results per chain; none of them calls pixel_of or reads a.batch_pixels, the
// frame's width or its shard. gi_total = n.
// STATS: the reference's tree; primary_rays / primary_hits count the roots, gather rays are in no ray counter (as in the frame path),
// their traversal counters are.
// Included by render_rays4.hip and render_rays5.hip only.
#ifndef RTU_RENDER_PATHS_IMPL_H_INCLUDED
#define RTU_RENDER_PATHS_IMPL_H_INCLUDED
// (render_impl.h defines the kernels of a camera's launch sequence, which nothing here launches)
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#pragma clang diagnostic ignored "-Wunused-function"
#include "render_impl.h"
#include "rtu_query.h"

namespace {

// (three wavefronts per SIMD, as k_ray_roots and the one-lane-per-ray stage-2 walks: RTU_OCC_WALK)
template <int STACK, bool STATS, int TEX>
__global__ void __launch_bounds__(64) RTU_OCC_WALK k_path_roots(KernelArgs a, const float4* __restrict__ rays) {
    __shared__ uint32_t s_stack[STACK * 64];
    const DevScene& s = a.scene;
    const uint32_t lane = threadIdx.x;
    const uint32_t n = a.gi_total;
    const uint32_t chunks = (n + 63u) / 64u;
    Counters cnt = {};
    for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint32_t i = c * 64u + lane;
        float4 ra = make_float4(0, 0, 0, 0), rb = ra;
        uint32_t key = 0;
        if (i < n) { ra = rays[2 * (size_t)i]; rb = rays[2 * (size_t)i + 1]; key = ray_keys(a)[i]; }
        const bool valid = i < n && ray_valid(ra, rb);
        if (i < n && !valid) {
            a.out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // not traced; t == 0 means nothing else (a valid ray has tmax > 0)
            a.gi_h[(size_t)n + i] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0u));  // no hit, at this depth and every deeper one
        }
        if (!valid) continue;
        Ray ray;
        ray.p = mk3(ra.x, ra.y, ra.z);
        ray.dir = mk3(rb.x, rb.y, rb.z);  // as given: not renormalised
        Hit h;
        fresh_hit(h, ra.w);
        h.uvw = mk3(0, 0, 0);
        RTU_CNT(prim);
        bool deferred;
        const bool hit = trace<STACK, STATS, !STATS, false, false, TEXD, false, false, false, true>(s, ray, false, h, s_stack + lane, cnt, deferred);  // FAR: any origin
        bool want = false;
        int mid = -1;
        if (!hit) {
            const f3 env = (TEXD && s.env.has_map) ? env_sample(s, ray.dir) : ld3(s.environment);
            a.out[i] = make_float4(env.x, env.y, env.z, h.z);  // h.z: still tmax
        } else {
            RTU_CNT(prim_hit);
            mid = as_const(s.nodes)[h.node].material_id;
            if (mid < 0) a.out[i] = make_float4(1.0f, 1.0f, 1.0f, h.z);  // null material => white
            else want = true;
        }
        // the chain's depth-0 record, as primary_pixel writes it for a pixel
        a.gi_h[i] = make_float4(h.p.x, h.p.y, h.p.z, h.z);
        a.gi_h[(size_t)n + i] = make_float4(h.N.x, h.N.y, h.N.z, __uint_as_float((want ? 1u : 0u) | (h.front ? 2u : 0u) | ((uint32_t)(mid + 1) << 2)));
        a.gi_h[2u * (size_t)n + i] = make_float4(ray.dir.x, ray.dir.y, ray.dir.z, __uint_as_float(key));
        if (TEXD) a.gi_h[3u * (size_t)n + i] = make_float4(h.uvw.x, h.uvw.y, h.uvw.z, 0.0f);
    }
    flush_counters<STATS>(a, cnt);
}

template <int STACK, bool STATS, int TEX>
__global__ void __launch_bounds__(64) RTU_OCC_WALK k_path_step(KernelArgs a) {
    __shared__ uint32_t s_stack[STACK * 64];
    const DevScene& s = a.scene;
    const uint32_t lane = threadIdx.x;
    const uint32_t n = a.gi_total;
    const uint32_t chunks = (n + 63u) / 64u;
    Counters cnt = {};
    for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint32_t i = c * 64u + lane;
        if (i >= n) continue;
        // the gather ray from the hit of depth k - 1 (RenderFunctions.cpp:556-565)
        const size_t hb = (size_t)(a.gi_depth - 1u) * 4u * n + i;
        const size_t ho = (size_t)a.gi_depth * 4u * n + i;
        const float4 hB = a.gi_h[hb + n];
        if (!(__float_as_uint(hB.w) & 1u)) {  // the chain ended above: no hit at this depth either (the rest of its record may never have been written)
            a.gi_h[ho + n] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0u));
            continue;
        }
        const float4 hA = a.gi_h[hb], hC = a.gi_h[hb + 2u * (size_t)n];
        const uint32_t pkey = __float_as_uint(hC.w);
        const f3 sampleOffset = sample_hemisphere_cosine(mk3(hB.x, hB.y, hB.z), pkey);
        Ray ray;
        ray.p = mk3(hA.x, hA.y, hA.z);
        ray.dir = norm3(sampleOffset);  // :562
        const uint32_t key = child_key(pkey, RTU_SLOT_GATHER);
        Hit h;
        fresh_hit(h, RTU_BIGFLOAT);
        h.uvw = mk3(0, 0, 0);
        bool deferred;
        const bool hit = trace<STACK, STATS, !STATS, false, false, TEXD, false>(s, ray, false, h, s_stack + lane, cnt, deferred);
        const int hmid = hit ? as_const(s.nodes)[h.node].material_id : -1;
        a.gi_h[ho] = make_float4(h.p.x, h.p.y, h.p.z, h.z);
        a.gi_h[ho + n] = make_float4(h.N.x, h.N.y, h.N.z, __uint_as_float((hit ? 1u : 0u) | (h.front ? 2u : 0u) | ((uint32_t)(hmid + 1) << 2)));
        a.gi_h[ho + 2u * (size_t)n] = make_float4(ray.dir.x, ray.dir.y, ray.dir.z, __uint_as_float(key));
        if (TEXD) a.gi_h[ho + 3u * (size_t)n] = make_float4(h.uvw.x, h.uvw.y, h.uvw.z, 0.0f);
    }
    flush_counters<STATS>(a, cnt);
}

// depth 0: the roots (rays != nullptr); depth 1 .. RTU_GI_BOUNCES: one chain step
template <int STACK, int TEX>
int launch_path_chain(const KernelArgs& a, const float4* rays, bool stats, hipStream_t stream) {
    if (a.gi_total == 0) return (int)hipSuccess;
    const uint32_t chunks = (a.gi_total + 63u) / 64u;
    const dim3 grid(chunks < 32768u ? chunks : 32768u);  // (the grid of the one-lane-per-ray walks: launch_all gridN)
    if (a.gi_depth == 0) {
        if (stats) hipLaunchKernelGGL((k_path_roots<STACK, true, TEX>), grid, dim3(64), 0, stream, a, rays);
        else hipLaunchKernelGGL((k_path_roots<STACK, false, TEX>), grid, dim3(64), 0, stream, a, rays);
    } else {
        if (stats) hipLaunchKernelGGL((k_path_step<STACK, true, TEX>), grid, dim3(64), 0, stream, a);
        else hipLaunchKernelGGL((k_path_step<STACK, false, TEX>), grid, dim3(64), 0, stream, a);
    }
    return (int)hipGetLastError();
}

template <int TEX>
int launch_path_chain_stack(const KernelArgs& a, const float4* rays, uint32_t bvh_stack_needed, bool stats, hipStream_t stream) {
    if (bvh_stack_needed <= 16) return launch_path_chain<16, TEX>(a, rays, stats, stream);
    if (bvh_stack_needed <= 24) return launch_path_chain<24, TEX>(a, rays, stats, stream);
    if (bvh_stack_needed <= 32) return launch_path_chain<32, TEX>(a, rays, stats, stream);
    return launch_path_chain<RTU_MAX_BVH_STACK, TEX>(a, rays, stats, stream);
}

}  // namespace

#endif
