// render_rays7.hip — k_gather_amb and k_irr_roots of render_gather_impl.h on a textured scene (feature set 3 | 8 | 32): the environment
// along a gather ray that missed may be a map, and the chain records carry uvw.
#include "render_gather_impl.h"

int rtu_launch_gather_amb7(const DevScene& s, const float4* gi_h, const float4* gi_res, uint32_t n, float4* out, hipStream_t stream) {
    return launch_gather_amb<3 | 8 | 32>(s, gi_h, gi_res, n, out, stream);
}

int rtu_launch_irr_roots7(const DevScene& s, const IrrRoots& r, uint32_t bvh_stack_needed, float4* gi_h, float4* out, hipStream_t stream) {
    return launch_irr_roots<3 | 8 | 32>(s, r, bvh_stack_needed, gi_h, out, stream);
}
