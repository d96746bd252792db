// rtu_raysort.hip — ray sorting (include/rtu_render.h, "Ray sorting"): the permutation that brings a batch of
// caller-supplied rays into a coherent order, and the kernels that apply it.
//
//   k_sort_keys      one key per ray (rtu_raysort.h: ray_sort_key; an invalid ray by ray_valid of rtu_query.h): two float4 loads per ray
//   k_sort_hist      per tile of RTU_SORT_TILE consecutive pairs: the histogram of one 8-bit digit, counted in LDS
//   k_sort_scan      per digit: the exclusive scan of its counts over the tiles, and the digit's total
//   k_sort_scatter   per tile: every pair to the place its digit, its tile and its rank inside the tile give it
//   k_permute*       dst[i] = src[order[i]] or dst[order[i]] = src[i] for elements of 1, 4 or 16 / 32 / 48 bytes (as float4 units)
//
// The sort is a least-significant-digit radix sort of (key, index) pairs, four passes of 8 bits over the 32-bit key (30 bits of
// cell and direction; a miss has bit 30 set, an invalid ray every bit). It is STABLE, so the result is argsort(keys, stable) whatever the
// grid: the histogram table is laid out digit-major [digit][tile], so its exclusive scan in that order is where each tile's run of
// each digit begins; inside a tile the four wavefronts take consecutive quarters and each wavefront its keys 64 at a time in
// order, ranking the lanes of one step by ballots (the lanes with the same digit, counted below the lane), the steps through a
// per-wavefront running count in LDS, and the wavefronts through a prefix over those counts. Nothing depends on the order in
// which workgroups or wavefronts happen to run. Every store is a vector store; there is no inline assembly.
#include "rtu_raysort.h"

#include "rtu_query.h"
#include "rtu_render.h"

namespace {

constexpr uint32_t kTile = RTU_SORT_TILE, kBins = RTU_SORT_BINS, kBlock = RTU_SORT_BLOCK, kWaves = kBlock / 64, kItems = RTU_SORT_ITEMS;
constexpr uint32_t kScanBlock = 256;  // k_sort_scan: threads per digit row
static_assert(kBins <= kBlock && kBins == kScanBlock, "thread d takes digit value d in the prefix steps");
static_assert(kWaves * 64 == kBlock && kBlock <= 1024, "tile geometry");

__global__ void __launch_bounds__(256) k_sort_keys(SortBox box, const float4* __restrict__ rays, uint32_t* __restrict__ keys, uint32_t n) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const float4 a = rays[2 * (size_t)i], b = rays[2 * (size_t)i + 1];
        uint32_t key = RTU_SORTKEY_INVALID;
        if (ray_valid(a, b)) {
            const float org[3] = {a.x, a.y, a.z}, dir[3] = {b.x, b.y, b.z};
            key = ray_sort_key(box, org, a.w, dir);
        }
        keys[i] = key;
    }
}

// hist[digit * tiles + tile] = pairs of tile `tile` whose key has that digit at `shift`
__global__ void __launch_bounds__(kBlock) k_sort_hist(const uint32_t* __restrict__ keys, uint32_t n, uint32_t shift, uint32_t tiles,
                                                      uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_hist[kBins];
    const uint32_t tile = blockIdx.x;
    if (threadIdx.x < kBins) s_hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = tile * kTile;
    for (uint32_t k = 0; k < kItems; k++) {
        const uint32_t i = base + k * kBlock + threadIdx.x;
        if (i < n) atomicAdd(&s_hist[(keys[i] >> shift) & (kBins - 1)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < kBins) hist[threadIdx.x * tiles + tile] = s_hist[threadIdx.x];
}

// exclusive scan of the values v (one per thread) over a workgroup of NW wavefronts; *total (may be nullptr) gets the sum. s_w: NW words.
template <uint32_t NW>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_w, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < NW; w++) {
        const uint32_t t = s_w[w];
        if (w < wave) before += t;
        all += t;
    }
    if (total) *total = all;
    __syncthreads();  // s_w may be reused
    return before + inc - v;
}

// one workgroup per digit: hist[digit][0 .. tiles) becomes its exclusive scan, totals[digit] its sum
__global__ void __launch_bounds__(kScanBlock) k_sort_scan(uint32_t* __restrict__ hist, uint32_t tiles, uint32_t* __restrict__ totals) {
    __shared__ uint32_t s_w[kScanBlock / 64];
    uint32_t* row = hist + (size_t)blockIdx.x * tiles;
    const uint32_t per = (tiles + kScanBlock - 1) / kScanBlock;
    const uint32_t t0 = threadIdx.x * per, t1 = t0 + per < tiles ? t0 + per : tiles;
    uint32_t sum = 0;
    for (uint32_t t = t0; t < t1; t++) sum += row[t];
    uint32_t all;
    uint32_t run = block_excl_scan<kScanBlock / 64>(sum, s_w, &all);
    for (uint32_t t = t0; t < t1; t++) {
        const uint32_t c = row[t];
        row[t] = run;
        run += c;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = all;
}

// FIRST: the pairs are (keys[i], i), idx_in is not read. LAST: keys_out is not written (the order is all that is left to want).
template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(kBlock) k_sort_scatter(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ idx_in, uint32_t n,
                                                         uint32_t shift, uint32_t tiles, const uint32_t* __restrict__ hist,
                                                         const uint32_t* __restrict__ totals, uint32_t* __restrict__ keys_out,
                                                         uint32_t* __restrict__ idx_out) {
    __shared__ uint32_t s_cnt[kWaves][kBins];  // per wavefront: pairs of each digit so far; then where the wavefront's run of it begins
    __shared__ uint32_t s_w[kWaves];
    const uint32_t tile = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t j = threadIdx.x; j < kWaves * kBins; j += kBlock) (&s_cnt[0][0])[j] = 0;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t base = tile * kTile + wave * (kItems * 64u);
    uint32_t key[kItems], off[kItems];
#pragma unroll
    for (uint32_t k = 0; k < kItems; k++) {
        const uint32_t i = base + k * 64u + lane;
        const bool live = i < n;
        key[k] = live ? keys_in[i] : 0u;
        const uint32_t digit = (key[k] >> shift) & (kBins - 1);
        // the live lanes of this step that hold the same digit
        unsigned long long same = __ballot(live);
#pragma unroll
        for (uint32_t b = 0; b < 8; b++) {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long vote = __ballot(bit);
            same &= bit ? vote : ~vote;
        }
        const uint32_t rank = (uint32_t)__popcll(same & below);
        const int leader = live ? __ffsll((long long)same) - 1 : 0;
        uint32_t before = 0;
        if (live && (int)lane == leader) before = atomicAdd(&s_cnt[wave][digit], (uint32_t)__popcll(same));  // this wavefront's row only
        before = __shfl(before, leader, 64);
        off[k] = before + rank;
    }
    __syncthreads();
    // thread d: where digit d begins overall (the scan over the digits' totals), plus this tile's place in the digit's run, then the
    // wavefronts of the tile in order
    {
        const uint32_t d = threadIdx.x;  // (threads beyond the digit values only take part in the scan, with nothing)
        uint32_t run = block_excl_scan<kWaves>(d < kBins ? totals[d] : 0u, s_w, nullptr);
        if (d < kBins) {
            run += hist[(size_t)d * tiles + tile];
            for (uint32_t w = 0; w < kWaves; w++) {
                const uint32_t c = s_cnt[w][d];
                s_cnt[w][d] = run;
                run += c;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kItems; k++) {
        const uint32_t i = base + k * 64u + lane;
        if (i >= n) continue;
        const uint32_t pos = s_cnt[wave][(key[k] >> shift) & (kBins - 1)] + off[k];
        if (pos >= n) continue;  // cannot happen while the histogram is that of these keys; never write outside the buffers
        if (!LAST) keys_out[pos] = key[k];
        idx_out[pos] = FIRST ? i : idx_in[i];
    }
}

template <class T>
__global__ void __launch_bounds__(256) k_permute(const T* __restrict__ src, T* __restrict__ dst, const uint32_t* __restrict__ order, size_t n,
                                                 int scatter) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        const size_t o = order[i];
        if (scatter) dst[o] = src[i];
        else dst[i] = src[o];
    }
}

// elements of U float4: one thread per float4, so that a wavefront moves whole elements with 16-byte accesses
template <uint32_t U>
__global__ void __launch_bounds__(256) k_permute16(const float4* __restrict__ src, float4* __restrict__ dst, const uint32_t* __restrict__ order,
                                                   size_t units, int scatter) {
    for (size_t j = (size_t)blockIdx.x * 256u + threadIdx.x; j < units; j += (size_t)gridDim.x * 256u) {
        const size_t e = j / U, c = j - e * U;
        const size_t o = (size_t)order[e] * U + c;
        if (scatter) dst[o] = src[j];
        else dst[j] = src[o];
    }
}

uint32_t grid_for(size_t threads) {
    const size_t blocks = (threads + 255) / 256;
    return (uint32_t)(blocks < 16384 ? blocks : 16384);
}

}  // namespace

size_t rtu_ray_order_scratch_words(size_t n) {
    const size_t tiles = (n + kTile - 1) / kTile;
    return 4 * n + (size_t)kBins * tiles + kBins;
}

int rtu_launch_ray_order(const SortBox& box, const float4* rays, size_t n, uint32_t* order, uint32_t* scratch, hipStream_t stream) {
    const uint32_t n32 = (uint32_t)n, tiles = (uint32_t)((n + kTile - 1) / kTile);
    uint32_t* key[2] = {scratch, scratch + n};
    uint32_t* idx[2] = {scratch + 2 * n, scratch + 3 * n};
    uint32_t* hist = scratch + 4 * n;
    uint32_t* totals = hist + (size_t)kBins * tiles;
    hipLaunchKernelGGL(k_sort_keys, dim3(grid_for(n)), dim3(256), 0, stream, box, rays, key[0], n32);
    for (uint32_t pass = 0; pass < 4; pass++) {
        const uint32_t shift = 8 * pass, in = pass & 1u, out = in ^ 1u;
        hipLaunchKernelGGL(k_sort_hist, dim3(tiles), dim3(kBlock), 0, stream, key[in], n32, shift, tiles, hist);
        hipLaunchKernelGGL(k_sort_scan, dim3(kBins), dim3(kScanBlock), 0, stream, hist, tiles, totals);
        if (pass == 0)
            hipLaunchKernelGGL((k_sort_scatter<true, false>), dim3(tiles), dim3(kBlock), 0, stream, key[in], idx[in], n32, shift, tiles, hist, totals,
                               key[out], idx[out]);
        else if (pass < 3)
            hipLaunchKernelGGL((k_sort_scatter<false, false>), dim3(tiles), dim3(kBlock), 0, stream, key[in], idx[in], n32, shift, tiles, hist, totals,
                               key[out], idx[out]);
        else
            hipLaunchKernelGGL((k_sort_scatter<false, true>), dim3(tiles), dim3(kBlock), 0, stream, key[in], idx[in], n32, shift, tiles, hist, totals,
                               key[out], order);
    }
    return (int)hipGetLastError();
}

int rtu_launch_permute(const void* src, void* dst, const uint32_t* order, size_t n, uint32_t elem_bytes, int scatter, hipStream_t stream) {
    if (n == 0) return (int)hipSuccess;
    const int sc = scatter ? 1 : 0;
    if (elem_bytes == 1)
        hipLaunchKernelGGL(k_permute<uint8_t>, dim3(grid_for(n)), dim3(256), 0, stream, (const uint8_t*)src, (uint8_t*)dst, order, n, sc);
    else if (elem_bytes == 4)
        hipLaunchKernelGGL(k_permute<uint32_t>, dim3(grid_for(n)), dim3(256), 0, stream, (const uint32_t*)src, (uint32_t*)dst, order, n, sc);
    else if (elem_bytes == 16)
        hipLaunchKernelGGL(k_permute16<1>, dim3(grid_for(n)), dim3(256), 0, stream, (const float4*)src, (float4*)dst, order, n, sc);
    else if (elem_bytes == 32)
        hipLaunchKernelGGL(k_permute16<2>, dim3(grid_for(2 * n)), dim3(256), 0, stream, (const float4*)src, (float4*)dst, order, 2 * n, sc);
    else
        hipLaunchKernelGGL(k_permute16<3>, dim3(grid_for(3 * n)), dim3(256), 0, stream, (const float4*)src, (float4*)dst, order, 3 * n, sc);
    return (int)hipGetLastError();
}

// ---- the key on the host (rtu_render.h: rtu_ray_sort_keys): ray_valid's rule restated for the host, then the same ray_sort_key ----
extern "C" int rtu_ray_sort_keys(const float box[6], const RtuRay* rays, size_t n, uint32_t* keys_out) {
    if (!box || (n && (!rays || !keys_out))) return RTU_ERR_ARG;
    const SortBox bx = make_sortbox(box);
    for (size_t i = 0; i < n; i++) {
        const RtuRay& r = rays[i];
        bool fin = sortbox_fin(r.tmax);
        for (int k = 0; k < 3; k++) fin = fin && sortbox_fin(r.org[k]) && sortbox_fin(r.dir[k]);
        const float dd = dot3(ld3(r.dir), ld3(r.dir));
        const bool valid = fin && r.tmax > 0.0f && !(fabsf(dd - 1.0f) > 2e-3f);
        keys_out[i] = valid ? ray_sort_key(bx, r.org, r.tmax, r.dir) : RTU_SORTKEY_INVALID;
    }
    return RTU_OK;
}
