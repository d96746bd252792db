// rtu_holes.hip — hole rays of include/rtu_render.h ("Hole rays"): the host forms rtu_hole_allocation and rtu_hole_fold, which are the
// executable statement of the rules, and the kernels of the two _device forms. Both call the same functions of rtu_holes.h and
// rtu_steer.h. (The rays are rtu_extra_sample_rays / k_steer_rays, unchanged.)
//
//   k_hole_weight   a workgroup per tile of 1024 pixels, four CONSECUTIVE pixels per lane: their four bytes of the hole plane (one
//                   dword load where the plane is 4-byte aligned and the four lie in the image, byte loads otherwise), the flags word
//                   of the hit record only where a byte is 1, the four weights out as one 16-byte store (the scratch k_steer_counts
//                   reads), and the tile's sum — at most 1024 — reduced over the workgroup and added to the 64-bit Wsum with ONE
//                   atomicAdd per workgroup. k_steer_counts, k_steer_sums and k_steer_finish of rtu_steer.hip follow, unchanged.
//   k_hole_fold     a lane per pixel: its count (one dword) and nothing more where that is 0 — almost everywhere once the history has
//                   filled —; else its offset, hole byte, hit flags, albedo and sample in, E, M, the image pixel and the hole byte out.
//
// Every store is a vector store, the one atomic a vector atomic; no LDS but the four words of the reduction, no inline assembly.
// Nothing is read or written beyond `pixels` or `n_rays`, whatever the counts and offsets hold.
#include "rtu_holes.h"

#include <vector>

namespace {

constexpr uint32_t kTile = 1024;  // pixels per workgroup of 256 lanes: the tiles of k_steer_counts

__global__ void __launch_bounds__(256) k_hole_weight(const uint8_t* __restrict__ hole, const float4* __restrict__ hits, uint32_t n,
                                                     uint32_t* __restrict__ w_out, unsigned long long* __restrict__ wsum) {
    __shared__ uint32_t s_w[4];
    const uint32_t p0 = blockIdx.x * kTile + 4u * threadIdx.x;
    uint32_t sum = 0;
    if (p0 < n) {
        uint32_t bytes = 0;  // byte k: hole[p0 + k], 0 beyond the image
        if (p0 + 4u <= n && (reinterpret_cast<uintptr_t>(hole) & 3u) == 0) {
            bytes = *reinterpret_cast<const uint32_t*>(hole + p0);
        } else {
            for (uint32_t k = 0; k < 4 && p0 + k < n; k++) bytes |= (uint32_t)hole[p0 + k] << (8u * k);
        }
        uint32_t w[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            w[k] = ((bytes >> (8u * k)) & 0xFFu) == 1u ? hl_weight(hits[3 * (size_t)(p0 + k)].z) : 0u;
            sum += w[k];
        }
        *reinterpret_cast<uint4*>(w_out + p0) = make_uint4(w[0], w[1], w[2], w[3]);  // (the scratch is padded to whole groups of four)
    }
    for (uint32_t d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
    if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t all = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
        if (all != 0u) atomicAdd(wsum, (unsigned long long)all);
    }
}

__global__ void __launch_bounds__(256) k_hole_fold(uint32_t n, float4* __restrict__ hist, float4* __restrict__ rgbz, uint8_t* __restrict__ hole,
                                                   const float4* __restrict__ hits, const float4* __restrict__ albedo,
                                                   const uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets,
                                                   const float4* __restrict__ rgbt, uint32_t n_rays) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    if (counts[p] == 0u) return;
    const uint32_t o = offsets[p];
    if (o >= n_rays) return;
    float4 E = hist[p], M = hist[3 * (size_t)n + p], img = rgbz[p];
    if (!hl_fold(hole[p], hits[3 * (size_t)p], albedo[p], rgbt[o], E, M, img)) return;
    hist[p] = E;
    hist[3 * (size_t)n + p] = M;
    rgbz[p] = img;
    hole[p] = 0;
}

}  // namespace

int rtu_launch_hole_allocation(const RtuHoleDesc& d, const uint8_t* hole, const float4* hits, uint32_t* counts, uint32_t* offsets, uint32_t* total,
                               uint32_t* scratch, hipStream_t stream) {
    const uint32_t n = (uint32_t)d.width * (uint32_t)d.height, tiles = (n + kTile - 1) / kTile;
    const StScratch s = st_scratch(scratch, n);
    const hipError_t e = hipMemsetAsync(scratch, 0, 16, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_hole_weight, dim3(tiles), dim3(256), 0, stream, hole, hits, n, s.w, s.wsum);
    return rtu_launch_allocation_scan(hl_steer_desc(d), s, counts, offsets, total, stream);
}

int rtu_launch_hole_fold(size_t pixels, float4* hist, float4* rgbz, uint8_t* hole, const float4* hits, const float4* albedo, const uint32_t* counts,
                         const uint32_t* offsets, const float4* rgbt, uint32_t n_rays, hipStream_t stream) {
    if (n_rays == 0) return (int)hipSuccess;
    const uint32_t n = (uint32_t)pixels;
    hipLaunchKernelGGL(k_hole_fold, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, hist, rgbz, hole, hits, albedo, counts, offsets, rgbt, n_rays);
    return (int)hipGetLastError();
}

int rtu_hole_check_desc(const RtuHoleDesc* d) {
    if (!d || d->width < 1 || d->height < 1 || d->width > 65536 || d->height > 65536) return RTU_ERR_ARG;
    if ((unsigned long long)d->width * (unsigned long long)d->height > (1ull << 26)) return RTU_ERR_ARG;
    if (d->budget > (1u << 26)) return RTU_ERR_ARG;
    for (uint32_t r : d->reserved)
        if (r) return RTU_ERR_ARG;
    return RTU_OK;
}

extern "C" {

int rtu_hole_defaults(RtuHoleDesc* out) {
    if (!out) return RTU_ERR_ARG;
    *out = RtuHoleDesc{};
    return RTU_OK;
}

int rtu_hole_allocation(const RtuHoleDesc* desc, const uint8_t* h_hole, const RtuRayHit* h_hits, uint32_t* counts, uint32_t* offsets, uint32_t* total) {
    if (rtu_hole_check_desc(desc) != RTU_OK || !h_hole || !h_hits || !counts || !offsets || !total) return RTU_ERR_ARG;
    const size_t n = (size_t)desc->width * (size_t)desc->height;
    const float* h = reinterpret_cast<const float*>(h_hits);
    std::vector<uint32_t> w(n);
    unsigned long long wsum = 0;
    for (size_t p = 0; p < n; p++) {
        w[p] = h_hole[p] == 1 ? hl_weight(h[12 * p + 2]) : 0u;
        wsum += w[p];
    }
    uint32_t run = 0;  // (at most 2^26)
    for (size_t p = 0; p < n; p++) {
        const uint32_t c = st_count((uint32_t)p, w[p], wsum, desc->budget, 1u, desc->frame_index);
        st_cut(c, run, desc->budget, counts[p], offsets[p]);
        run += c;
    }
    *total = run < desc->budget ? run : desc->budget;
    return RTU_OK;
}

int rtu_hole_fold(const RtuHoleDesc* desc, float* h_hist, float* h_rgbz, uint8_t* h_hole, const RtuRayHit* h_hits, const float* h_albedo,
                  const uint32_t* counts, const uint32_t* offsets, const float* h_rgbt, size_t n_rays) {
    if (rtu_hole_check_desc(desc) != RTU_OK || !h_hist || !h_rgbz || !h_hole || !h_hits || !h_albedo || !counts || !offsets || (n_rays && !h_rgbt))
        return RTU_ERR_ARG;
    if (n_rays > ((size_t)1 << 26)) return RTU_ERR_ARG;
    const size_t n = (size_t)desc->width * (size_t)desc->height;
    for (size_t p = 0; p < n; p++)
        if (counts[p] > 1u || (unsigned long long)offsets[p] + counts[p] > n_rays) return RTU_ERR_ARG;  // a sample outside h_rgbt
    const float* h = reinterpret_cast<const float*>(h_hits);
    for (size_t p = 0; p < n; p++) {
        if (counts[p] == 0u) continue;
        float4 E = f4(h_hist, p), M = f4(h_hist, 3 * n + p), img = f4(h_rgbz, p);
        if (!hl_fold(h_hole[p], f4(h, 3 * p), f4(h_albedo, p), f4(h_rgbt, offsets[p]), E, M, img)) continue;
        st4(h_hist, p, E);
        st4(h_hist, 3 * n + p, M);
        st4(h_rgbz, p, img);
        h_hole[p] = 0;
    }
    return RTU_OK;
}

}  // extern "C"
