// render_rays6.hip — the two halves of a recipe-P sample along caller-supplied rays and the roots of an irradiance-map pass
// (render_gather_impl.h) on an untextured scene (feature set 2 | 8 | 32), the launch interface of both scene kinds (rtu_irradiance.h),
// and k_amb_seed, which knows no scene.
#include "render_gather_impl.h"

namespace {

// per chain: "the gather ray of depth 1 hit material 0, and its two Shade() trees gave {amb, 0}" — what k_gi_roots at depth 0 reads
__global__ void __launch_bounds__(256) k_amb_seed(float4* __restrict__ gi_h, float4* __restrict__ gi_res, const float4* __restrict__ amb, uint32_t total) {
    const uint32_t chain = blockIdx.x * 256u + threadIdx.x;
    if (chain >= total) return;
    const size_t n = total;
    const float4 c = amb[chain];
    gi_h[(size_t)5u * n + chain] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(1u | (1u << 2)));
    gi_res[chain] = make_float4(c.x, c.y, c.z, 0.0f);
    gi_res[n + chain] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

}  // namespace

int rtu_launch_gather_amb7(const DevScene& s, const float4* gi_h, const float4* gi_res, uint32_t n, float4* out, hipStream_t stream);
int rtu_launch_irr_roots7(const DevScene& s, const IrrRoots& r, uint32_t bvh_stack_needed, float4* gi_h, float4* out, hipStream_t stream);

int rtu_launch_gather_amb(const DevScene& s, const float4* gi_h, const float4* gi_res, uint32_t n, float4* out, hipStream_t stream) {
    return s.textured ? rtu_launch_gather_amb7(s, gi_h, gi_res, n, out, stream) : launch_gather_amb<2 | 8 | 32>(s, gi_h, gi_res, n, out, stream);
}

int rtu_launch_irr_roots(const DevScene& s, const IrrRoots& r, uint32_t bvh_stack_needed, float4* gi_h, float4* out, hipStream_t stream) {
    return s.textured ? rtu_launch_irr_roots7(s, r, bvh_stack_needed, gi_h, out, stream)
                      : launch_irr_roots<2 | 8 | 32>(s, r, bvh_stack_needed, gi_h, out, stream);
}

int rtu_launch_amb_seed(float4* gi_h, float4* gi_res, const float4* amb, uint32_t n, hipStream_t stream) {
    if (n == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_amb_seed, dim3((n + 255u) / 256u), dim3(256), 0, stream, gi_h, gi_res, amb, n);
    return (int)hipGetLastError();
}
