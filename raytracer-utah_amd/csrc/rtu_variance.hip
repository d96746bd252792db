// rtu_variance.hip — the variance-guided preview filter of include/rtu_render.h ("Variance-guided filtering"): its host forms
// rtu_variance and rtu_denoise_variance, which are the executable statement of the rules, and the kernels of their _device forms.
// Both call the same functions of rtu_variance.h, pixel by pixel. (The moments they read are accumulated by rtu_temporal.hip.)
//
//   k_variance          one lane per pixel: its E, M and the first float4 of its RtuRayHit in, one float out. Only a lane whose history is
//                       shorter than min_history walks the 7 x 7 window (five 16-byte loads per usable tap); the other lanes of its
//                       wavefront wait for it and do nothing else.
//   k_vd_prepare        one lane per pixel: the caller's {rgbz, RtuRayHit, albedo, v} -> the planes gN, gP and e0
//   k_vd_pass           k_dn_pass of rtu_denoise.hip with the colour term of rtu_variance.h: the same lanes and workgroups, three
//                       16-byte loads per tap, and nine pairs of 4-byte loads per pixel for g3. Two IEEE divisions per tap where
//                       k_dn_pass has four — which by itself bought nothing: with k_dn_pass's loop (a tap's loads behind the tests
//                       of the tap before) a pass measured 0.207 ms at 1920 x 1080 against k_dn_pass's 0.184. The reading, from
//                       these timings alone and without counters: what binds such a pass is the latency of 25 dependent rounds of
//                       loads. vd_pass_pixel therefore loads every tap of a row
//                       unconditionally, from a clamped address, and skips by selects on the sums: the five taps of a row are in
//                       flight together, 0.169 ms per pass. LAST: the pass writes the output image instead
//                       of a plane.
// A pass reads plane e[i & 1] and writes e[(i + 1) & 1]; only the last touches rgbz_out, each lane its own pixel after reading that
// pixel of rgbz_in — so rgbz_out == rgbz_in is allowed.
#include "rtu_variance.h"

#include <vector>

namespace {

__global__ void __launch_bounds__(256) k_variance(VrParams V, const float4* __restrict__ hist, const float4* __restrict__ hits, float* __restrict__ v) {
    const int x = (int)(blockIdx.x * 32u + (threadIdx.x & 31u)), y = (int)(blockIdx.y * 8u + (threadIdx.x >> 5));
    if (x >= V.width || y >= V.height) return;
    const size_t n = (size_t)V.width * (size_t)V.height;
    v[(size_t)y * (size_t)V.width + (size_t)x] = vr_variance_pixel(V, hist, hist + 3 * n, hits, x, y);
}

__global__ void __launch_bounds__(256) k_vd_prepare(const float4* __restrict__ rgbz, const float4* __restrict__ hits, const float4* __restrict__ albedo,
                                                    const float* __restrict__ v, float sigma_plane, float4* __restrict__ gN, float4* __restrict__ gP,
                                                    float4* __restrict__ e, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (i >= n) return;
    const float4 hit[3] = {hits[3 * i], hits[3 * i + 1], hits[3 * i + 2]};
    float4 n4, p4, e4;
    vd_prepare(rgbz[i], hit, albedo[i], v[i], sigma_plane, n4, p4, e4);
    gN[i] = n4;
    gP[i] = p4;
    e[i] = e4;
}

template <bool LAST>
__global__ void __launch_bounds__(256) k_vd_pass(const float4* __restrict__ gN, const float4* __restrict__ gP, const float4* __restrict__ e_in,
                                                 float4* __restrict__ e_out, const float4* rgbz_in, const float4* __restrict__ albedo, float4* rgbz_out,
                                                 int width, int height, int step, float sl2, int nlog2) {
    const int x = (int)(blockIdx.x * 32u + (threadIdx.x & 31u)), y = (int)(blockIdx.y * 8u + (threadIdx.x >> 5));
    if (x >= width || y >= height) return;
    const size_t p = (size_t)y * (size_t)width + (size_t)x;
    const bool valid = gN[p].w != 0.0f;
    float4 e = e_in[p];
    if (valid) e = vd_pass_pixel(gN, gP, e_in, width, height, x, y, step, sl2, nlog2);
    if (LAST) rgbz_out[p] = dn_output(rgbz_in[p], albedo[p], valid, e);
    else e_out[p] = e;
}

}  // namespace

int rtu_launch_variance(const VrParams& V, const float4* hist, const float4* hits, float* v, hipStream_t stream) {
    const dim3 grid((uint32_t)((V.width + 31) / 32), (uint32_t)((V.height + 7) / 8));
    hipLaunchKernelGGL(k_variance, grid, dim3(256), 0, stream, V, hist, hits, v);
    return (int)hipGetLastError();
}

int rtu_launch_denoise_variance(const RtuVarianceDesc& desc, const float4* rgbz_in, const float4* hits, const float4* albedo, const float* v,
                                float4* rgbz_out, float4* planes, hipStream_t stream) {
    const unsigned long long n = (unsigned long long)desc.width * (unsigned long long)desc.height;
    float4* gN = planes;
    float4* gP = planes + n;
    float4* e[2] = {planes + 2 * n, planes + 3 * n};
    hipLaunchKernelGGL(k_vd_prepare, dim3((uint32_t)((n + 255ull) / 256ull)), dim3(256), 0, stream, rgbz_in, hits, albedo, v, desc.sigma_plane, gN, gP, e[0], n);
    const dim3 grid((uint32_t)((desc.width + 31) / 32), (uint32_t)((desc.height + 7) / 8));
    const float sl2 = desc.sigma_lum * desc.sigma_lum;
    for (int i = 0; i < desc.n_passes; i++) {
        if (i == desc.n_passes - 1)
            hipLaunchKernelGGL(k_vd_pass<true>, grid, dim3(256), 0, stream, gN, gP, e[i & 1], (float4*)nullptr, rgbz_in, albedo, rgbz_out, desc.width,
                               desc.height, 1 << i, sl2, desc.normal_log2_power);
        else
            hipLaunchKernelGGL(k_vd_pass<false>, grid, dim3(256), 0, stream, gN, gP, e[i & 1], e[(i + 1) & 1], (const float4*)nullptr,
                               (const float4*)nullptr, (float4*)nullptr, desc.width, desc.height, 1 << i, sl2, desc.normal_log2_power);
    }
    return (int)hipGetLastError();
}

int rtu_variance_check_desc(const RtuVarianceDesc* d) {
    if (!d || d->width < 1 || d->height < 1 || d->width > 65536 || d->height > 65536) return RTU_ERR_ARG;
    if ((unsigned long long)d->width * (unsigned long long)d->height > (1ull << 26)) return RTU_ERR_ARG;
    if (d->n_passes < 1 || d->n_passes > 8 || d->normal_log2_power < 0 || d->normal_log2_power > 7) return RTU_ERR_ARG;
    if (!(d->sigma_lum > 0.0f) || !(d->sigma_plane > 0.0f)) return RTU_ERR_ARG;  // a NaN is refused too
    if (d->min_history < 1 || d->min_history > 65535) return RTU_ERR_ARG;
    if (d->reserved[0] || d->reserved[1] || d->reserved[2]) return RTU_ERR_ARG;
    return RTU_OK;
}

extern "C" {

int rtu_variance_defaults(RtuVarianceDesc* out) {
    if (!out) return RTU_ERR_ARG;
    *out = RtuVarianceDesc{};
    out->n_passes = 3;
    out->sigma_lum = 2.0f;
    out->sigma_plane = 0.05f;
    out->normal_log2_power = 5;
    out->min_history = 4;
    return RTU_OK;
}

int rtu_variance(const RtuVarianceDesc* desc, const float* h_hist, const RtuRayHit* h_hits, float* h_v) {
    if (rtu_variance_check_desc(desc) != RTU_OK || !h_hist || !h_hits || !h_v) return RTU_ERR_ARG;
    const int W = desc->width, H = desc->height;
    const size_t n = (size_t)W * (size_t)H;
    std::vector<float4> E(n), M(n), hits(3 * n);
    const float* h = reinterpret_cast<const float*>(h_hits);
    for (size_t i = 0; i < n; i++) {
        E[i] = f4(h_hist, i);
        M[i] = f4(h_hist, 3 * n + i);
    }
    for (size_t i = 0; i < 3 * n; i++) hits[i] = f4(h, i);
    const VrParams V = vr_setup(*desc);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) h_v[(size_t)y * (size_t)W + (size_t)x] = vr_variance_pixel(V, E.data(), M.data(), hits.data(), x, y);
    return RTU_OK;
}

int rtu_denoise_variance(const RtuVarianceDesc* desc, const float* h_rgbz_in, const RtuRayHit* h_hits, const float* h_albedo, const float* h_v,
                         float* h_rgbz_out) {
    if (rtu_variance_check_desc(desc) != RTU_OK || !h_rgbz_in || !h_hits || !h_albedo || !h_v || !h_rgbz_out) return RTU_ERR_ARG;
    const int W = desc->width, H = desc->height;
    const size_t n = (size_t)W * (size_t)H;
    std::vector<float4> gN(n), gP(n), e0(n), e1(n);
    for (size_t i = 0; i < n; i++) {
        const float* h = reinterpret_cast<const float*>(h_hits + i);
        const float4 hit[3] = {f4(h, 0), f4(h, 1), f4(h, 2)};
        vd_prepare(f4(h_rgbz_in, i), hit, f4(h_albedo, i), h_v[i], desc->sigma_plane, gN[i], gP[i], e0[i]);
    }
    const float sl2 = desc->sigma_lum * desc->sigma_lum;
    std::vector<float4>* e[2] = {&e0, &e1};
    for (int i = 0; i < desc->n_passes; i++) {
        const std::vector<float4>& in = *e[i & 1];
        std::vector<float4>& out = *e[(i + 1) & 1];
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const size_t p = (size_t)y * (size_t)W + (size_t)x;
                out[p] = gN[p].w != 0.0f ? vd_pass_pixel(gN.data(), gP.data(), in.data(), W, H, x, y, 1 << i, sl2, desc->normal_log2_power) : in[p];
            }
    }
    const std::vector<float4>& last = *e[desc->n_passes & 1];
    for (size_t i = 0; i < n; i++)  // (the input pixel is read before the output pixel is written: h_rgbz_out may be h_rgbz_in)
        st4(h_rgbz_out, i, dn_output(f4(h_rgbz_in, i), f4(h_albedo, i), gN[i].w != 0.0f, last[i]));
    return RTU_OK;
}

}  // extern "C"
