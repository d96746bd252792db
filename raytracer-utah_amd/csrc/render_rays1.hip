// render_rays1.hip — a ray batch on feature set 1 (recipe W, textured): k_ray_roots of render_rays_impl.h, then the recursion
// levels of render_feat1.hip in the mode "roots are already queued on this stream" (launch_all, RTU_LAUNCH_LEVELS).
#include "render_rays_impl.h"

int rtu_launch_feat1(const KernelArgs& args, uint32_t n_tiles, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, int mode, const LaunchProbe* probe);

int rtu_launch_rays1(const KernelArgs& args, const float4* rays, uint32_t n, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, const LaunchProbe* probe) {
    const int e = launch_ray_roots_stack<1>(args, rays, n, bvh_stack_needed, stats, stream);
    if (e != (int)hipSuccess) return e;
    return rtu_launch_feat1(args, (n + 63u) / 64u, bvh_stack_needed, stats, stream, RTU_LAUNCH_LEVELS, probe);
}
