// rtu_steer.hip — steered sampling of include/rtu_render.h ("Steered sampling"): the host forms rtu_sample_allocation and
// rtu_temporal_refine, which are the executable statement of the rules, and the kernels of the three _device forms. Both call the
// same functions of rtu_steer.h. (rtu_extra_sample_rays, the third host form, is in rtu_capi_temporal.hip, built on cam_sample as rtu_camera_sample_rays is.)
//
//   k_steer_weight   a workgroup per tile of 1024 pixels, four pixels per lane 256 apart: E, M, v and the first float4 of the RtuRayHit
//                    in, the weight out (4 B per pixel of scratch), and the tile's sum — below 2^30 — reduced over the workgroup and
//                    added to the 64-bit Wsum with ONE atomicAdd per workgroup. The sum is exact, so its order does not matter.
//   k_steer_counts   the same tiles, four CONSECUTIVE pixels per lane (one 16-byte load of their weights): the counts before the
//                    cut, their exclusive scan inside the tile (the scan's first step) and the tile's sum
//   k_steer_sums     one workgroup: the exclusive scan of the at most 65536 tile sums, and the total before the cut
//   k_steer_finish   a lane per pixel: the tile's base added, the cut at the budget (st_cut), counts, offsets and the total written
//   k_steer_rays     a lane per pixel: its at most 15 rays, keys and owners written at its offset. Neighbouring lanes write
//                    neighbouring rays (the offsets rise with the pixel), and no lane has to search for its pixel.
//   k_refine         a lane per pixel: its samples folded into E, M and the image in place
//
// rtu_launch_allocation_scan launches k_steer_counts, k_steer_sums and k_steer_finish behind weights that are already in the scratch:
// rtu_launch_sample_allocation calls it behind k_steer_weight, "Hole rays" (rtu_holes.hip) behind a weight kernel of its own.
//
// Every store is a vector store, the one atomic a vector atomic; there is no inline assembly. Nothing is read or written beyond
// `pixels`, `capacity` or `n_rays`, whatever the counts and offsets hold.
#include "rtu_steer.h"

#include "rtu_intersect.h"

#include <vector>

namespace {

constexpr uint32_t kTile = 1024;  // pixels per workgroup of 256 lanes

struct DevSinCos {
    __device__ __forceinline__ void operator()(float t, float& sn, float& cs) const { portable_sincos(t, sn, cs); }
};

// exclusive scan of the values v (one per thread) over a workgroup of four wavefronts; all: their sum. s_w: four words.
__device__ __forceinline__ uint32_t st_block_excl_scan(uint32_t v, uint32_t* s_w, uint32_t& all) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    all = 0;
    for (uint32_t w = 0; w < 4; w++) {
        const uint32_t t = s_w[w];
        if (w < wave) before += t;
        all += t;
    }
    __syncthreads();  // s_w may be reused
    return before + inc - v;
}

__global__ void __launch_bounds__(256) k_steer_weight(const float4* __restrict__ hist, const float4* __restrict__ hits, const float* __restrict__ v,
                                                      uint32_t n, uint32_t* __restrict__ w_out, unsigned long long* __restrict__ wsum) {
    __shared__ uint32_t s_w[4];
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t p = blockIdx.x * kTile + k * 256u + threadIdx.x;
        if (p < n) {
            const uint32_t w = st_weight(hits[3 * (size_t)p], hist[p], hist[3 * (size_t)n + p], v[p]);
            w_out[p] = w;
            sum += w;
        }
    }
    uint32_t all;
    (void)st_block_excl_scan(sum, s_w, all);
    if (threadIdx.x == 0 && all != 0u) atomicAdd(wsum, (unsigned long long)all);
}

__global__ void __launch_bounds__(256) k_steer_counts(RtuSteerDesc d, const uint32_t* __restrict__ w_in, const unsigned long long* __restrict__ wsum,
                                                      uint32_t n, uint32_t* __restrict__ counts, uint32_t* __restrict__ offsets,
                                                      uint32_t* __restrict__ sums) {
    __shared__ uint32_t s_w[4];
    const unsigned long long ws = *wsum;
    const uint32_t p0 = blockIdx.x * kTile + 4u * threadIdx.x;
    uint4 w4 = make_uint4(0u, 0u, 0u, 0u);
    if (p0 < n) w4 = *reinterpret_cast<const uint4*>(w_in + p0);  // (the scratch is padded to whole groups of four)
    const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
    uint32_t c[4], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        c[k] = p0 + k < n ? st_count(p0 + k, w[k], ws, d.budget, (uint32_t)d.max_extra, d.frame_index) : 0u;
        sum += c[k];
    }
    uint32_t all;
    uint32_t run = st_block_excl_scan(sum, s_w, all);
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        if (p0 + k < n) {
            counts[p0 + k] = c[k];
            offsets[p0 + k] = run;
        }
        run += c[k];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = all;
}

__global__ void __launch_bounds__(256) k_steer_sums(uint32_t* __restrict__ sums, uint32_t tiles, uint32_t* __restrict__ raw_total) {
    __shared__ uint32_t s_w[4];
    const uint32_t per = (tiles + 255u) / 256u;
    const uint32_t t0 = threadIdx.x * per < tiles ? threadIdx.x * per : tiles, t1 = t0 + per < tiles ? t0 + per : tiles;
    uint32_t sum = 0;
    for (uint32_t t = t0; t < t1; t++) sum += sums[t];
    uint32_t all;
    uint32_t run = st_block_excl_scan(sum, s_w, all);
    for (uint32_t t = t0; t < t1; t++) {
        const uint32_t c = sums[t];
        sums[t] = run;
        run += c;
    }
    if (threadIdx.x == 0) *raw_total = all;
}

__global__ void __launch_bounds__(256) k_steer_finish(uint32_t budget, const uint32_t* __restrict__ sums, const uint32_t* __restrict__ raw_total, uint32_t n,
                                                      uint32_t* __restrict__ counts, uint32_t* __restrict__ offsets, uint32_t* __restrict__ total) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p == 0) {
        const uint32_t all = *raw_total;
        *total = all < budget ? all : budget;
    }
    if (p >= n) return;
    uint32_t c, o;
    st_cut(counts[p], offsets[p] + sums[p / kTile], budget, c, o);
    counts[p] = c;
    offsets[p] = o;
}

__global__ void __launch_bounds__(256) k_steer_rays(StRays r, uint32_t max_extra, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets,
                                                    float4* __restrict__ rays, uint32_t* __restrict__ keys, uint32_t* __restrict__ owner,
                                                    uint32_t capacity) {
    const uint32_t pixels = (uint32_t)r.c.width * (uint32_t)r.c.height;
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= pixels) return;
    const uint32_t cp = counts[p], o = offsets[p];
    const uint32_t c = cp < max_extra ? cp : max_extra;
    const uint32_t y = p / (uint32_t)r.c.width, x = p - y * (uint32_t)r.c.width;
    for (uint32_t j = 0; j < c; j++) {
        const unsigned long long i = (unsigned long long)o + j;
        if (i >= (unsigned long long)capacity) break;
        f3 org, dir;
        uint32_t key;
        st_extra_ray(r.c, r.ox[j], r.oy[j], r.sample0 + j, (int)x, (int)y, DevSinCos(), org, dir, key);
        rays[2 * i] = make_float4(org.x, org.y, org.z, RTU_BIGFLOAT);
        rays[2 * i + 1] = make_float4(dir.x, dir.y, dir.z, __uint_as_float(0u));
        keys[i] = key;
        owner[i] = p;
    }
}

__global__ void __launch_bounds__(256) k_refine(uint32_t n, float max_history, float4* __restrict__ hist, const float4* __restrict__ hits,
                                                const float4* __restrict__ albedo, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets,
                                                const float4* __restrict__ rgbt, uint32_t n_rays, float4* __restrict__ rgbz) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint32_t o = offsets[p] < n_rays ? offsets[p] : n_rays;
    const uint32_t room = n_rays - o, c = counts[p] < room ? counts[p] : room;
    if (c == 0u) return;
    float4 E = hist[p], M = hist[3 * (size_t)n + p], img = rgbz[p];
    if (!st_refine_pixel(max_history, hits[3 * (size_t)p], albedo[p], c, rgbt + o, E, M, img)) return;
    hist[p] = E;
    hist[3 * (size_t)n + p] = M;
    rgbz[p] = img;
}

}  // namespace

size_t rtu_steer_scratch_words(size_t pixels) {
    const size_t tiles = (pixels + kTile - 1) / kTile;
    return 4 + 4 * ((pixels + 3) / 4) + tiles;
}

int rtu_launch_allocation_scan(const RtuSteerDesc& d, const StScratch& s, uint32_t* counts, uint32_t* offsets, uint32_t* total, hipStream_t stream) {
    const uint32_t n = (uint32_t)d.width * (uint32_t)d.height, tiles = (n + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_steer_counts, dim3(tiles), dim3(256), 0, stream, d, s.w, s.wsum, n, counts, offsets, s.sums);
    hipLaunchKernelGGL(k_steer_sums, dim3(1), dim3(256), 0, stream, s.sums, tiles, s.raw_total);
    hipLaunchKernelGGL(k_steer_finish, dim3((n + 255u) / 256u), dim3(256), 0, stream, d.budget, s.sums, s.raw_total, n, counts, offsets, total);
    return (int)hipGetLastError();
}

int rtu_launch_sample_allocation(const RtuSteerDesc& d, const float4* hist, const float4* hits, const float* v, uint32_t* counts, uint32_t* offsets,
                                 uint32_t* total, uint32_t* scratch, hipStream_t stream) {
    const uint32_t n = (uint32_t)d.width * (uint32_t)d.height, tiles = (n + kTile - 1) / kTile;
    const StScratch s = st_scratch(scratch, n);
    const hipError_t e = hipMemsetAsync(scratch, 0, 16, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_steer_weight, dim3(tiles), dim3(256), 0, stream, hist, hits, v, n, s.w, s.wsum);
    return rtu_launch_allocation_scan(d, s, counts, offsets, total, stream);
}

int rtu_launch_extra_sample_rays(const StRays& r, uint32_t max_extra, const uint32_t* counts, const uint32_t* offsets, float4* rays, uint32_t* keys,
                                 uint32_t* owner, uint32_t capacity, hipStream_t stream) {
    const uint32_t pixels = (uint32_t)r.c.width * (uint32_t)r.c.height;
    if (capacity == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_steer_rays, dim3((pixels + 255u) / 256u), dim3(256), 0, stream, r, max_extra, counts, offsets, rays, keys, owner, capacity);
    return (int)hipGetLastError();
}

int rtu_launch_temporal_refine(size_t pixels, float max_history, float4* hist, const float4* hits, const float4* albedo, const uint32_t* counts,
                               const uint32_t* offsets, const float4* rgbt, uint32_t n_rays, float4* rgbz, hipStream_t stream) {
    if (n_rays == 0) return (int)hipSuccess;
    const uint32_t n = (uint32_t)pixels;
    hipLaunchKernelGGL(k_refine, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, max_history, hist, hits, albedo, counts, offsets, rgbt, n_rays, rgbz);
    return (int)hipGetLastError();
}

int rtu_steer_check_desc(const RtuSteerDesc* d) {
    if (!d || d->width < 1 || d->height < 1 || d->width > 65536 || d->height > 65536) return RTU_ERR_ARG;
    if ((unsigned long long)d->width * (unsigned long long)d->height > (1ull << 26)) return RTU_ERR_ARG;
    if (d->budget > (1u << 26) || d->max_extra < 1 || d->max_extra > ST_MAX_EXTRA) return RTU_ERR_ARG;
    if (d->reserved[0] || d->reserved[1] || d->reserved[2]) return RTU_ERR_ARG;
    return RTU_OK;
}

extern "C" {

int rtu_steer_defaults(RtuSteerDesc* out) {
    if (!out) return RTU_ERR_ARG;
    *out = RtuSteerDesc{};
    out->max_extra = 3;
    return RTU_OK;
}

int rtu_sample_allocation(const RtuSteerDesc* desc, const float* h_hist, const RtuRayHit* h_hits, const float* h_v, uint32_t* counts, uint32_t* offsets,
                          uint32_t* total) {
    if (rtu_steer_check_desc(desc) != RTU_OK || !h_hist || !h_hits || !h_v || !counts || !offsets || !total) return RTU_ERR_ARG;
    const size_t n = (size_t)desc->width * (size_t)desc->height;
    const float* h = reinterpret_cast<const float*>(h_hits);
    std::vector<uint32_t> w(n);
    unsigned long long wsum = 0;
    for (size_t p = 0; p < n; p++) {
        w[p] = st_weight(f4(h, 3 * p), f4(h_hist, p), f4(h_hist, 3 * n + p), h_v[p]);
        wsum += w[p];
    }
    uint32_t run = 0;  // (at most 15 * 2^26)
    for (size_t p = 0; p < n; p++) {
        const uint32_t c = st_count((uint32_t)p, w[p], wsum, desc->budget, (uint32_t)desc->max_extra, desc->frame_index);
        st_cut(c, run, desc->budget, counts[p], offsets[p]);
        run += c;
    }
    *total = run < desc->budget ? run : desc->budget;
    return RTU_OK;
}

int rtu_temporal_refine(const RtuTemporalDesc* desc, float* h_hist, const RtuRayHit* h_hits, const float* h_albedo, const uint32_t* counts,
                        const uint32_t* offsets, const float* h_rgbt, size_t n_rays, float* h_rgbz) {
    if (rtu_temporal_check_desc(desc) != RTU_OK || !h_hist || !h_hits || !h_albedo || !counts || !offsets || !h_rgbz || (n_rays && !h_rgbt)) return RTU_ERR_ARG;
    if (n_rays > ((size_t)1 << 26)) return RTU_ERR_ARG;
    const size_t n = (size_t)desc->width * (size_t)desc->height;
    for (size_t p = 0; p < n; p++)
        if ((unsigned long long)offsets[p] + counts[p] > n_rays) return RTU_ERR_ARG;  // a sample outside h_rgbt
    const float* h = reinterpret_cast<const float*>(h_hits);
    std::vector<float4> samples;
    for (size_t p = 0; p < n; p++) {
        samples.resize(counts[p]);
        for (uint32_t j = 0; j < counts[p]; j++) samples[j] = f4(h_rgbt, (size_t)offsets[p] + j);
        float4 E = f4(h_hist, p), M = f4(h_hist, 3 * n + p), img = f4(h_rgbz, p);
        if (!st_refine_pixel((float)desc->max_history, f4(h, 3 * p), f4(h_albedo, p), counts[p], samples.data(), E, M, img)) continue;
        st4(h_hist, p, E);
        st4(h_hist, 3 * n + p, M);
        st4(h_rgbz, p, img);
    }
    return RTU_OK;
}

}  // extern "C"
