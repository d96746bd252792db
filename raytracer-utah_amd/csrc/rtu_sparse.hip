// rtu_sparse.hip — sparse sessions of include/rtu_render.h ("Sparse sessions"): the host form rtu_sparse_fill, which is the executable
// statement of the fill, and the kernels of the _device forms. Both call the same functions of rtu_sparse.h. (rtu_sparse_rays, the host
// form of the rays, is in rtu_capi_temporal.hip beside rtu_extra_sample_rays; the sparse accumulator is k_temporal<true, true, false, true> of
// rtu_temporal.hip.)
//
//   k_sparse_rays   a lane per block: its owner of the frame, and that pixel's ray and key in the sample the block has reached, as two
//                   float4 stores and two dword stores. The camera and the offsets of the (at most four) samples are kernel arguments.
//   k_sparse_fill   a lane per pixel, 32 x 8 pixel workgroups as k_temporal. A lane reads its byte of the hole plane and ends unless it
//                   is 1; a hole reads its own guides (64 B) and, of up to nine blocks, the owner (one dword), the sample (16 B) and the
//                   owner's guides (up to 64 B), and writes its float4 of the image. Holes are few once the history has filled, and
//                   are whole regions right after a cut: there neighbouring lanes visit the same blocks, so the lines are shared
//                   through the vector L1.
//
// Every store is a vector store; no LDS, no atomics, no inline assembly. Nothing is read or written beyond the blocks and the pixels of
// the image, whatever `owner` holds.
#include "rtu_sparse.h"

#include "rtu_intersect.h"

#include <vector>

namespace {

struct DevSinCos {
    __device__ __forceinline__ void operator()(float t, float& sn, float& cs) const { portable_sincos(t, sn, cs); }
};

__global__ void __launch_bounds__(256) k_sparse_rays(SpRays R, float4* __restrict__ rays, uint32_t* __restrict__ keys, uint32_t* __restrict__ owner) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= R.blocks) return;
    f3 org, dir;
    uint32_t key, own;
    sp_ray(R, b, DevSinCos(), org, dir, key, own);
    rays[2 * (size_t)b] = make_float4(org.x, org.y, org.z, RTU_BIGFLOAT);
    rays[2 * (size_t)b + 1] = make_float4(dir.x, dir.y, dir.z, __uint_as_float(0u));
    keys[b] = key;
    owner[b] = own;
}

__global__ void __launch_bounds__(256) k_sparse_fill(SpFill F, const float4* __restrict__ hits, const float4* __restrict__ albedo,
                                                     const uint32_t* __restrict__ owner, const float4* __restrict__ rgbt,
                                                     const uint8_t* __restrict__ hole, float4* rgbz) {
    const int x = (int)(blockIdx.x * 32u + (threadIdx.x & 31u)), y = (int)(blockIdx.y * 8u + (threadIdx.x >> 5));
    if (x >= F.width || y >= F.height) return;
    const size_t p = (size_t)y * (size_t)F.width + (size_t)x;
    if (hole[p] != 1) return;
    rgbz[p] = sp_fill(F, x, y, hits, albedo, owner, rgbt, rgbz[p]);
}

}  // namespace

int rtu_launch_sparse_rays(const SpRays& r, float4* rays, uint32_t* keys, uint32_t* owner, hipStream_t stream) {
    if (r.blocks == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_sparse_rays, dim3((r.blocks + 255u) / 256u), dim3(256), 0, stream, r, rays, keys, owner);
    return (int)hipGetLastError();
}

int rtu_launch_sparse_fill(const SpFill& f, const float4* hits, const float4* albedo, const uint32_t* owner, const float4* rgbt, const uint8_t* hole,
                           float4* rgbz, hipStream_t stream) {
    const dim3 grid((uint32_t)((f.width + 31) / 32), (uint32_t)((f.height + 7) / 8));
    hipLaunchKernelGGL(k_sparse_fill, grid, dim3(256), 0, stream, f, hits, albedo, owner, rgbt, hole, rgbz);
    return (int)hipGetLastError();
}

int rtu_sparse_check_desc(const RtuSparseDesc* d) {
    if (!d || d->width < 1 || d->height < 1 || d->width > 65536 || d->height > 65536) return RTU_ERR_ARG;
    if ((unsigned long long)d->width * (unsigned long long)d->height > (1ull << 26)) return RTU_ERR_ARG;
    if (d->block < 1 || d->block > SP_MAX_BLOCK) return RTU_ERR_ARG;
    for (uint32_t r : d->reserved)
        if (r) return RTU_ERR_ARG;
    return RTU_OK;
}

extern "C" {

int rtu_sparse_defaults(RtuSparseDesc* out) {
    if (!out) return RTU_ERR_ARG;
    *out = RtuSparseDesc{};
    out->block = 2;
    return RTU_OK;
}

int rtu_sparse_fill(const RtuTemporalDesc* desc, const RtuSparseDesc* sparse_desc, const RtuRayHit* h_hits, const float* h_albedo, const uint32_t* owner,
                    const float* h_rgbt, const uint8_t* h_hole, float* h_rgbz) {
    if (rtu_temporal_check_desc(desc) != RTU_OK || rtu_sparse_check_desc(sparse_desc) != RTU_OK || sparse_desc->width != desc->width ||
        sparse_desc->height != desc->height)
        return RTU_ERR_ARG;
    if (!h_hits || !h_albedo || !owner || !h_rgbt || !h_hole || !h_rgbz) return RTU_ERR_ARG;
    const int W = desc->width, H = desc->height, B = sparse_desc->block;
    const SpFill F{W, H, B, sp_blocks(W, B), sp_blocks(H, B), desc->sigma_plane, desc->normal_min};
    const size_t n = (size_t)W * (size_t)H, blocks = (size_t)F.sw * (size_t)F.sh;
    for (size_t b = 0; b < blocks; b++)
        if ((size_t)owner[b] >= n) return RTU_ERR_ARG;
    // (the guides and the samples as float4: the caller's floats need not be 16-byte aligned)
    std::vector<float4> hits(3 * n), albedo(n), rgbt(blocks);
    const float* h = reinterpret_cast<const float*>(h_hits);
    for (size_t i = 0; i < 3 * n; i++) hits[i] = f4(h, i);
    for (size_t i = 0; i < n; i++) albedo[i] = f4(h_albedo, i);
    for (size_t i = 0; i < blocks; i++) rgbt[i] = f4(h_rgbt, i);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * (size_t)W + (size_t)x;
            if (h_hole[p] != 1) continue;
            st4(h_rgbz, p, sp_fill(F, x, y, hits.data(), albedo.data(), owner, rgbt.data(), f4(h_rgbz, p)));
        }
    return RTU_OK;
}

}  // extern "C"
