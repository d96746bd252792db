// render_rays5.hip — the front of a PATH-TRACED ray batch (rtu_shade_rays_paths) on a textured scene (recipe P; feature set
// 3 | 8 | 32): k_path_roots and k_path_step of render_paths_impl.h with uvw in the chain records and a mapped environment. The
// Shade() trees behind the chain are the kernels of render_feat11.hip as compiled.
#include "render_paths_impl.h"

int rtu_launch_paths5(const KernelArgs& args, const float4* rays, uint32_t bvh_stack_needed, bool stats, hipStream_t stream) {
    return launch_path_chain_stack<3 | 8 | 32>(args, rays, bvh_stack_needed, stats, stream);
}
