// render_rays2.hip — a SAMPLED ray batch (rtu_shade_rays_sampled) on feature set 2 | 32 (recipe S, untextured; RAYD): k_ray_roots of
// render_rays_impl.h with the caller's key per ray, then the recursion levels instantiated HERE (launch_all, RTU_LAUNCH_LEVELS) — the
// level kernels of render_feat2.hip derive a level-0 frame's key from its pixel (frame_smp), these read it from the key buffer.
#include "render_rays_impl.h"

namespace {
int launch_levels2(const KernelArgs& args, uint32_t n_chunks, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, const LaunchProbe* probe) {
    if (bvh_stack_needed <= 16) return launch_all<16, 2 | 32>(args, n_chunks, stats, stream, RTU_LAUNCH_LEVELS, probe);
    if (bvh_stack_needed <= 24) return launch_all<24, 2 | 32>(args, n_chunks, stats, stream, RTU_LAUNCH_LEVELS, probe);
    if (bvh_stack_needed <= 32) return launch_all<32, 2 | 32>(args, n_chunks, stats, stream, RTU_LAUNCH_LEVELS, probe);
    return launch_all<RTU_MAX_BVH_STACK, 2 | 32>(args, n_chunks, stats, stream, RTU_LAUNCH_LEVELS, probe);
}
}  // namespace

int rtu_launch_rays2(const KernelArgs& args, const float4* rays, uint32_t n, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, const LaunchProbe* probe) {
    const int e = launch_ray_roots_stack<2 | 32>(args, rays, n, bvh_stack_needed, stats, stream);
    if (e != (int)hipSuccess) return e;
    return launch_levels2(args, (n + 63u) / 64u, bvh_stack_needed, stats, stream, probe);
}

int rtu_launch_rays3(const KernelArgs& args, const float4* rays, uint32_t n, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, const LaunchProbe* probe);

// (rtu_device.h) the dispatch of a sampled ray batch: args.cam carries the keys (ray_keys), args.sampling is set
int rtu_launch_ray_batch_sampled(const KernelArgs& args, const float4* rays, uint32_t n, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, const LaunchProbe* probe) {
    if (!args.sampling || args.frame_batch || !args.cam) return (int)hipErrorInvalidValue;  // recipe S with a key per ray, nothing else
    return args.scene.textured ? rtu_launch_rays3(args, rays, n, bvh_stack_needed, stats, stream, probe)
                               : rtu_launch_rays2(args, rays, n, bvh_stack_needed, stats, stream, probe);
}
