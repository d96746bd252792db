// render_rays3.hip — a SAMPLED ray batch (rtu_shade_rays_sampled) on feature set 3 | 32 (recipe S, textured; RAYD): k_ray_roots of
// render_rays_impl.h with the caller's key per ray, then the recursion levels instantiated here (see render_rays2.hip).
#include "render_rays_impl.h"

namespace {
int launch_levels3(const KernelArgs& args, uint32_t n_chunks, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, const LaunchProbe* probe) {
    if (bvh_stack_needed <= 16) return launch_all<16, 3 | 32>(args, n_chunks, stats, stream, RTU_LAUNCH_LEVELS, probe);
    if (bvh_stack_needed <= 24) return launch_all<24, 3 | 32>(args, n_chunks, stats, stream, RTU_LAUNCH_LEVELS, probe);
    if (bvh_stack_needed <= 32) return launch_all<32, 3 | 32>(args, n_chunks, stats, stream, RTU_LAUNCH_LEVELS, probe);
    return launch_all<RTU_MAX_BVH_STACK, 3 | 32>(args, n_chunks, stats, stream, RTU_LAUNCH_LEVELS, probe);
}
}  // namespace

int rtu_launch_rays3(const KernelArgs& args, const float4* rays, uint32_t n, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, const LaunchProbe* probe) {
    const int e = launch_ray_roots_stack<3 | 32>(args, rays, n, bvh_stack_needed, stats, stream);
    if (e != (int)hipSuccess) return e;
    return launch_levels3(args, (n + 63u) / 64u, bvh_stack_needed, stats, stream, probe);
}
