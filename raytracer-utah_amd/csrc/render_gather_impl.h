// render_gather_impl.h — THE TWO HALVES OF A RECIPE-P SAMPLE along caller-supplied rays (rtu_gather_rays / rtu_shade_rays_ambient,
// include/rtu_render.h) and the roots of an irradiance-map pass (rtu_irradiance_build, rtu_irradiance.h). A recipe-P sample is
// Shade(h0, AmbientLight(c)) + Shade(h0, lights) (RenderFunctions.cpp:134-135), c being what MonteCarlo(h0, 4) gathered (:549-590).
// The path-traced ray batch (render_paths_impl.h) computes c inside k_gi_roots at depth 0 and consumes it there. Here:
//
//   k_gather_amb<TEX>          the `amb` of k_gi_roots for k == 0 (render_impl.h) WRITTEN OUT: behind the roots, the four chain steps and
//                              the shading steps of depth 4 .. 1 of a path-traced batch — all as compiled —, chain i reads the depth-1 hit
//                              flag and, by it, the two results of depth 1, white twice, or the environment along the gather ray, and
//                              writes {c, t} to out[i]. A chain without a shaded depth-0 hit (miss, invalid ray, node without material)
//                              gets c = 0 and keeps the t k_path_roots wrote. The same three expressions in the same order as
//                              k_gi_roots: shade_rays_ambient of these c is shade_rays_paths byte for byte (tests/test_gpu_irradiance_rays.py).
//   k_amb_seed                 the other half needs NO kernel of the launch sequence compiled again: behind k_path_roots it writes, per
//                              chain, a depth-1 record that says "hit, material 0" and the two results {amb[i], 0}; k_gi_roots at depth 0
//                              — as compiled — then forms (0 + amb[i]) + 0, which is MonteCarlo()'s own sum (:568-570) and amb[i] bit for
//                              bit (but for a negative zero), and shades the two trees of :134-135. No chain step runs. 48 bytes per ray
//                              of traffic instead of a second instantiation of the 106-SGPR kernels.
//   k_irr_roots<STACK, TEX>    k_path_roots for the listed points of an irradiance-map pass: one lane per POINT traces the pinhole ray
//                              through the point's pixel corner once and writes M depth-0 chain records that differ in their key only,
//                              rtu_sample_key(point index, first_sample + m). A miss writes z = tmax and N = 0 into its records, which
//                              k_irr_store copies into the map.
// Included by render_rays6.hip (untextured scenes) and render_rays7.hip (textured ones) only.
#ifndef RTU_RENDER_GATHER_IMPL_H_INCLUDED
#define RTU_RENDER_GATHER_IMPL_H_INCLUDED
// (render_impl.h defines the kernels of a camera's launch sequence, which nothing here launches)
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#pragma clang diagnostic ignored "-Wunused-function"
#include "render_impl.h"
#include "rtu_irradiance.h"
#include "rtu_query.h"

namespace {

template <int TEX>
__global__ void __launch_bounds__(256) k_gather_amb(DevScene s, const float4* __restrict__ gi_h, const float4* __restrict__ gi_res, uint32_t total,
                                                    float4* __restrict__ out) {
    const uint32_t chain = blockIdx.x * 256u + threadIdx.x;
    if (chain >= total) return;
    const size_t n = total;
    const uint32_t pk = __float_as_uint(gi_h[n + chain].w);
    if (!(pk & 1u) || (int)(pk >> 2) - 1 < 0) {  // nothing is shaded at depth 0: nothing was gathered for it; t is the roots'
        out[chain] = make_float4(0.0f, 0.0f, 0.0f, out[chain].w);
        return;
    }
    // render_impl.h k_gi_roots, k == 0 < RTU_GI_BOUNCES
    f3 amb;
    const size_t hn = (size_t)4u * n + chain;
    const uint32_t npk = __float_as_uint(gi_h[hn + n].w);
    if (npk & 1u) {
        if ((int)(npk >> 2) - 1 < 0) {
            amb = (mk3(0, 0, 0) + mk3(1, 1, 1)) + mk3(1, 1, 1);  // a node without material shades white, twice
        } else {
            const float4 ra = gi_res[chain], rd = gi_res[n + chain];
            amb = (mk3(0, 0, 0) + mk3(ra.x, ra.y, ra.z)) + mk3(rd.x, rd.y, rd.z);  // :569-570
        }
    } else {
        const float4 nd = gi_h[hn + 2u * n];
        amb = mk3(0, 0, 0) + ((TEXD && s.env.has_map) ? env_sample(s, mk3(nd.x, nd.y, nd.z)) : ld3(s.environment));  // :575
    }
    out[chain] = make_float4(amb.x, amb.y, amb.z, gi_h[chain].w);
}

// (three wavefronts per SIMD, as k_path_roots)
template <int STACK, int TEX>
__global__ void __launch_bounds__(64) RTU_OCC_WALK k_irr_roots(DevScene s, IrrRoots r, float4* __restrict__ gi_h, float4* __restrict__ out) {
    constexpr bool STATS = false;
    __shared__ uint32_t s_stack[STACK * 64];
    const uint32_t lane = threadIdx.x;
    const size_t n = (size_t)r.n_points * r.samples;  // chains
    const uint32_t chunks = (r.n_points + 63u) / 64u;
    Counters cnt = {};
    for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint32_t j = c * 64u + lane;
        if (j >= r.n_points) continue;
        const uint32_t point = r.list[j];
        Ray ray;
        irr_point_ray(r.cam, point, ray.p, ray.dir);
        Hit h;
        fresh_hit(h, RTU_BIGFLOAT);
        h.uvw = mk3(0, 0, 0);
        bool deferred;
        const bool hit = trace<STACK, STATS, !STATS, false, false, TEXD, false, false, false, true>(s, ray, false, h, s_stack + lane, cnt, deferred);
        int mid = -1;
        if (hit) mid = as_const(s.nodes)[h.node].material_id;
        else h.N = mk3(0, 0, 0);  // (h.z: still tmax)
        const bool want = hit && mid >= 0;
        const float4 rA = make_float4(h.p.x, h.p.y, h.p.z, h.z), rD = make_float4(h.uvw.x, h.uvw.y, h.uvw.z, 0.0f);
        const float4 rB = make_float4(h.N.x, h.N.y, h.N.z, __uint_as_float((want ? 1u : 0u) | (h.front ? 2u : 0u) | ((uint32_t)(mid + 1) << 2)));
        for (uint32_t m = 0; m < r.samples; m++) {
            const size_t i = (size_t)j * r.samples + m;
            gi_h[i] = rA;
            gi_h[n + i] = rB;
            gi_h[2u * n + i] = make_float4(ray.dir.x, ray.dir.y, ray.dir.z, __uint_as_float(cs_sample_key(point, r.first_sample + m)));
            if (TEXD) gi_h[3u * n + i] = rD;
            if (!want) out[i] = make_float4(0.0f, 0.0f, 0.0f, h.z);
        }
    }
}

template <int TEX>
int launch_gather_amb(const DevScene& s, const float4* gi_h, const float4* gi_res, uint32_t n, float4* out, hipStream_t stream) {
    if (n == 0) return (int)hipSuccess;
    hipLaunchKernelGGL((k_gather_amb<TEX>), dim3((n + 255u) / 256u), dim3(256), 0, stream, s, gi_h, gi_res, n, out);
    return (int)hipGetLastError();
}

template <int STACK, int TEX>
int launch_irr_roots_stack(const DevScene& s, const IrrRoots& r, float4* gi_h, float4* out, hipStream_t stream) {
    if (r.n_points == 0 || r.samples == 0) return (int)hipSuccess;
    const uint32_t chunks = (r.n_points + 63u) / 64u;
    hipLaunchKernelGGL((k_irr_roots<STACK, TEX>), dim3(chunks < 32768u ? chunks : 32768u), dim3(64), 0, stream, s, r, gi_h, out);
    return (int)hipGetLastError();
}

template <int TEX>
int launch_irr_roots(const DevScene& s, const IrrRoots& r, uint32_t bvh_stack_needed, float4* gi_h, float4* out, hipStream_t stream) {
    if (bvh_stack_needed <= 16) return launch_irr_roots_stack<16, TEX>(s, r, gi_h, out, stream);
    if (bvh_stack_needed <= 24) return launch_irr_roots_stack<24, TEX>(s, r, gi_h, out, stream);
    if (bvh_stack_needed <= 32) return launch_irr_roots_stack<32, TEX>(s, r, gi_h, out, stream);
    return launch_irr_roots_stack<RTU_MAX_BVH_STACK, TEX>(s, r, gi_h, out, stream);
}

}  // namespace

#endif
