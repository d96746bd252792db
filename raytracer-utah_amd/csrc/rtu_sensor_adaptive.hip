// rtu_sensor_adaptive.hip — adaptive sensors (include/rtu_render.h, "Adaptive sensors"): the layer between the sensor's
// rays (rtu_sensor.h) and the ray-batch launch path — a list of the pixels that still sample, the rays of that list, and the stopping
// rule applied in sample order to what comes back.
//
//   k_sa_rays<MODEL>  one lane per (sample of the batch, entry of the live list): the ray of rtu_sensor.h's sensor_ray for pixel list[i]
//                     as two float4 stores and its key as one dword store, at index k * live_n + i. blockIdx.y is the sample of the
//                     launch: every live pixel has taken the same number of samples, so the offsets and the sample index are
//                     wave-uniform (scalar loads from the kernel arguments), as in k_sensor_rays. The first batch is dense and is
//                     written by k_sensor_rays itself.
//   k_sa_step         one lane per live entry: the samples of the batch in sample order, one float4 load each, added to the pixel's
//                     sums; the rule at every checkpoint the batch crosses. A pixel that passes stops there — the rest of the batch is
//                     not read —, and its mean and count are written at once. The survivors of a block are packed in lane order
//                     (ballot + popcount per wavefront, four counts through LDS), their number goes to blk[block].
//   k_sa_scan         one block: the exclusive scan of the per-block counts; the total is the next list's length.
//   k_sa_gather       one block per block of k_sa_step: its packed survivors to their place in the next list, which so stays in
//                     ascending pixel order whatever the order the blocks ran in.
//
// No atomics, no float min / max; every store is a vector store; there is no inline assembly. Where the frame counters report a batch
// that the host will shade again (skip_if), all three kernels return at once and change nothing.
#include "rtu_sensor_adaptive.h"

#include "rtu_intersect.h"

namespace {

struct DevSinCos {
    __device__ __forceinline__ void operator()(float t, float& sn, float& cs) const { portable_sincos(t, sn, cs); }
};

template <int MODEL>
__global__ void __launch_bounds__(256) k_sa_rays(RtuSensorDesc d, SensorOffsets off, const uint32_t* __restrict__ list, uint32_t live_n,
                                                  float4* __restrict__ rays, uint32_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= live_n) return;
    const uint32_t s = blockIdx.y;
    const uint32_t p = list[i];
    const uint32_t y = p / (uint32_t)d.width, x = p - y * (uint32_t)d.width;
    f3 org, dir;
    sensor_ray<MODEL>(d, (int)x, (int)y, off.ox[s], off.oy[s], DevSinCos(), org, dir);
    const size_t r = (size_t)s * live_n + i;
    rays[2 * r] = make_float4(org.x, org.y, org.z, RTU_BIGFLOAT);
    rays[2 * r + 1] = make_float4(dir.x, dir.y, dir.z, __uint_as_float(0u));
    keys[r] = sample_key(p, off.sample[s]);
}

__device__ __forceinline__ bool sa_skip(const SaStep& p) { return (p.skip_if[0] | p.skip_if[1] | p.skip_if_side[0] | p.skip_if_side[1]) != 0u; }

// var <= target for one channel: (q - s * (s / n)) / (n - 1), every operation rounded (this file is compiled with -ffp-contract=off)
__device__ __forceinline__ bool sa_agrees(float s, float q, float n, float target) { return (q - s * (s / n)) / (n - 1.0f) <= target; }

__global__ void __launch_bounds__(256) k_sa_step(SaStep p) {
    if (sa_skip(p)) return;  // (uniform: before the barrier)
    __shared__ uint32_t wave_n[4];
    const uint32_t i = blockIdx.x * RTU_SA_BLOCK + threadIdx.x;
    bool live = i < p.live_n;
    uint32_t pix = 0;
    float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q = s;
    uint32_t h = 0;
    if (live) {
        pix = p.list ? p.list[i] : i;
        if (p.done) {
            s = p.s[pix];
            q = p.q[pix];
            h = __float_as_uint(q.w);
        }
    }
    uint32_t cp = p.checkpoint;
    for (uint32_t b = 0; b < p.batch; b++) {  // (b, n and cp are uniform: a stopped lane is masked, it does not leave the loop)
        const uint32_t n = p.done + b + 1u;
        const bool check = n == cp && n < p.max_samples;
        if (n == cp) cp += p.increment;
        if (!live) continue;
        const float4 v = p.samples[(size_t)b * p.live_n + i];
        s.x += v.x; s.y += v.y; s.z += v.z;
        q.x += v.x * v.x; q.y += v.y * v.y; q.z += v.z * v.z;
        if (v.w != RTU_BIGFLOAT && v.w != 0.0f) { s.w += v.w; h++; }  // a miss answers tmax, a sample outside the fisheye circle 0
        bool stop = n == p.max_samples;
        if (check) {
            const float nf = (float)n;
            stop = n == 1u ? p.target == __uint_as_float(0x7f800000u)  // var = +inf
                           : sa_agrees(s.x, q.x, nf, p.target) && sa_agrees(s.y, q.y, nf, p.target) && sa_agrees(s.z, q.z, nf, p.target);
        }
        if (stop) {
            const float nf = (float)n;
            p.out[pix] = make_float4(s.x / nf, s.y / nf, s.z / nf, h ? s.w / (float)h : RTU_BIGFLOAT);
            if (p.counts) p.counts[pix] = (uint8_t)n;
            live = false;
        }
    }
    if (live) {
        q.w = __uint_as_float(h);
        p.s[pix] = s;
        p.q[pix] = q;
    }
    // the survivors of the block, packed in lane order
    const unsigned long long m = __ballot(live);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) wave_n[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < wave; w++) base += wave_n[w];
    if (live) p.packed[(size_t)blockIdx.x * RTU_SA_BLOCK + base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = pix;
    if (threadIdx.x == 0u) p.blk[blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}

// blk[nb + j] = the sum of blk[0 .. j) for j < nb, *n_out = the sum of all: one block of 1024 lanes, a run of consecutive counts each
__global__ void __launch_bounds__(1024) k_sa_scan(SaStep p, uint32_t nb) {
    if (sa_skip(p)) return;
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t run = (nb + 1023u) / 1024u;
    const uint32_t lo = t * run < nb ? t * run : nb, hi = lo + run < nb ? lo + run : nb;
    uint32_t sum = 0;
    for (uint32_t j = lo; j < hi; j++) sum += p.blk[j];
    part[t] = sum;
    __syncthreads();
    for (uint32_t o = 1; o < 1024u; o <<= 1) {
        const uint32_t v = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t at = part[t] - sum;
    for (uint32_t j = lo; j < hi; j++) {
        p.blk[nb + j] = at;
        at += p.blk[j];
    }
    if (t == 1023u) *p.n_out = part[1023];
}

__global__ void __launch_bounds__(256) k_sa_gather(SaStep p, uint32_t nb) {
    if (sa_skip(p)) return;
    const uint32_t n = p.blk[blockIdx.x], at = p.blk[nb + blockIdx.x];
    if (threadIdx.x < n) p.list_out[at + threadIdx.x] = p.packed[(size_t)blockIdx.x * RTU_SA_BLOCK + threadIdx.x];
}

}  // namespace

int rtu_launch_sa_rays(const RtuSensorDesc& d, const SensorOffsets& off, uint32_t n_samples, const uint32_t* list, uint32_t live_n, float4* rays,
                       uint32_t* keys, hipStream_t stream) {
    if (live_n == 0 || n_samples == 0) return (int)hipSuccess;
    const dim3 grid((live_n + 255u) / 256u, n_samples), block(256);
    switch (d.model) {
    case RTU_SENSOR_EQUIRECT: hipLaunchKernelGGL(k_sa_rays<RTU_SENSOR_EQUIRECT>, grid, block, 0, stream, d, off, list, live_n, rays, keys); break;
    case RTU_SENSOR_FISHEYE: hipLaunchKernelGGL(k_sa_rays<RTU_SENSOR_FISHEYE>, grid, block, 0, stream, d, off, list, live_n, rays, keys); break;
    default: hipLaunchKernelGGL(k_sa_rays<RTU_SENSOR_ORTHO>, grid, block, 0, stream, d, off, list, live_n, rays, keys); break;
    }
    return (int)hipGetLastError();
}

int rtu_launch_sa_step(const SaStep& p, hipStream_t stream) {
    if (p.live_n == 0) return (int)hipSuccess;
    const uint32_t nb = rtu_sa_blocks(p.live_n);
    hipLaunchKernelGGL(k_sa_step, dim3(nb), dim3(RTU_SA_BLOCK), 0, stream, p);
    hipLaunchKernelGGL(k_sa_scan, dim3(1), dim3(1024), 0, stream, p, nb);
    hipLaunchKernelGGL(k_sa_gather, dim3(nb), dim3(RTU_SA_BLOCK), 0, stream, p, nb);
    return (int)hipGetLastError();
}
