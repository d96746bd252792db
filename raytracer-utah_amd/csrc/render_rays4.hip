// render_rays4.hip — the front of a PATH-TRACED ray batch (rtu_shade_rays_paths) on an untextured scene (recipe P; feature set
// 2 | 8 | 32): k_path_roots and k_path_step of render_paths_impl.h. The Shade() trees behind the chain are the kernels of
// render_feat10.hip as compiled (rtu_launch_frame, RTU_LAUNCH_SHADE).
#include "render_paths_impl.h"

int rtu_launch_paths4(const KernelArgs& args, const float4* rays, uint32_t bvh_stack_needed, bool stats, hipStream_t stream) {
    return launch_path_chain_stack<2 | 8 | 32>(args, rays, bvh_stack_needed, stats, stream);
}

int rtu_launch_paths5(const KernelArgs& args, const float4* rays, uint32_t bvh_stack_needed, bool stats, hipStream_t stream);

// (rtu_device.h) one step of the chain of a path-traced ray batch: args.gi_depth 0 the roots, 1 .. RTU_GI_BOUNCES a gather ray
int rtu_launch_ray_batch_chain(const KernelArgs& args, const float4* rays, uint32_t bvh_stack_needed, bool stats, hipStream_t stream) {
    if (!args.sampling || args.frame_batch || !args.cam || !args.gi_h || args.gi_depth > (uint32_t)RTU_GI_BOUNCES || (args.gi_depth == 0 && !rays))
        return (int)hipErrorInvalidValue;  // recipe P with a key per ray, nothing else
    return args.scene.textured ? rtu_launch_paths5(args, rays, bvh_stack_needed, stats, stream)
                               : rtu_launch_paths4(args, rays, bvh_stack_needed, stats, stream);
}
