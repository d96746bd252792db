// rtu_mesh_update.hip — the device side of rtu_update_meshes (rtu_capi.hip): what a mesh's structures take from its vertices,
// rewritten in HBM from the f / v arrays already there. The arithmetic is rtu_meshrec.h's, shared with the host builders.
//   k_mu_tri_records   a lane per element slot: its 64-byte triangle record
//   k_mu_leaf_boxes    a lane per child slot of a collapsed tree: a leaf slot's box from the vertices of its element slots
//   k_mu_inner_boxes   a lane per child slot of one tree level: an inner slot's box from the node it refers to; launched level by
//                      level from the deepest up (nodes are breadth-first, so a level is a range of nodes)
// A few thousand lanes each: plain kernels, no LDS, no atomics. Every index a lane follows was range-checked on the host (faces and
// element ids at upload / by rtu_update_meshes, ref words are the upload's own).
#include "rtu_meshrec.h"

namespace {

const uint32_t kBlock = 256;

__global__ void k_mu_tri_records(const uint32_t* __restrict__ f, const float* __restrict__ v, const uint32_t* __restrict__ elements, uint32_t n,
                                 float4* __restrict__ tri) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    float4 r[4];
    mu_slot_record(f, v, elements, e, r);
    for (int i = 0; i < 4; i++) tri[4 * (size_t)e + i] = r[i];
}

template <int W>
__global__ void k_mu_leaf_boxes(float* tree, uint32_t n_nodes, const uint32_t* __restrict__ f, const float* __restrict__ v,
                                const uint32_t* __restrict__ elements, uint32_t n_elements) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes * (uint32_t)W) return;
    mu_leaf_slot<W>(tree, i / (uint32_t)W, i % (uint32_t)W, f, v, elements, n_elements);
}

template <int W>
__global__ void k_mu_inner_boxes(float* tree, uint32_t n_nodes, uint32_t node0, uint32_t node1) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (node1 - node0) * (uint32_t)W) return;
    mu_inner_slot<W>(tree, n_nodes, node0 + i / (uint32_t)W, i % (uint32_t)W);
}

template <int W>
hipError_t refit(hipStream_t st, float* tree, uint32_t n_nodes, const uint32_t* level_start, uint32_t n_levels, const uint32_t* f, const float* v,
                 const uint32_t* elements, uint32_t n_elements) {
    if (n_nodes == 0) return hipSuccess;
    const uint32_t slots = n_nodes * (uint32_t)W;
    k_mu_leaf_boxes<W><<<(slots + kBlock - 1) / kBlock, kBlock, 0, st>>>(tree, n_nodes, f, v, elements, n_elements);
    for (uint32_t L = n_levels; L-- > 0;) {  // (the deepest level has no inner slot: its launch finds nothing to do)
        const uint32_t node0 = level_start[L], node1 = level_start[L + 1];
        if (node1 <= node0 || node1 > n_nodes) continue;
        const uint32_t lanes = (node1 - node0) * (uint32_t)W;
        k_mu_inner_boxes<W><<<(lanes + kBlock - 1) / kBlock, kBlock, 0, st>>>(tree, n_nodes, node0, node1);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t mu_tri_records(hipStream_t st, const uint32_t* f, const float* v, const uint32_t* elements, uint32_t n, float4* tri) {
    if (n == 0) return hipSuccess;
    k_mu_tri_records<<<(n + kBlock - 1) / kBlock, kBlock, 0, st>>>(f, v, elements, n, tri);
    return hipGetLastError();
}

hipError_t mu_refit(hipStream_t st, int width, float4* tree, uint32_t n_nodes, const uint32_t* level_start, uint32_t n_levels, const uint32_t* f,
                    const float* v, const uint32_t* elements, uint32_t n_elements) {
    float* t = reinterpret_cast<float*>(tree);
    return width == 4 ? refit<4>(st, t, n_nodes, level_start, n_levels, f, v, elements, n_elements)
                      : refit<8>(st, t, n_nodes, level_start, n_levels, f, v, elements, n_elements);
}
