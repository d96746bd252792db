// rtu_denoise.hip — the denoising filter of include/rtu_render.h ("Denoising"): its host form rtu_denoise, which is the executable
// statement of the rules, and the kernels of rtu_denoise_device. Both call the same functions of rtu_denoise.h, pixel by pixel.
//
//   k_dn_prepare   one lane per pixel: the caller's {rgbz, RtuRayHit, albedo} -> the planes gN, gP and e0 (64 B read, 48 B written)
//   k_dn_pass      one lane per pixel, 32 x 8 pixel workgroups (a wavefront is two rows of 32: its taps of one (dx, dy) are two runs of
//                  512 B at step 1, and runs of 16 B lines at any step — the planes are float4, so a tap is three 16-byte loads
//                  whatever the step). The 25 taps of a workgroup's pixels overlap almost entirely for the small steps and are
//                  served by the vector L1 / L2; at the large steps every tap is its own line. Measured at 1920 x 1080, a pass
//                  takes the same 0.17 - 0.20 ms at every step: its four IEEE divisions per tap bind it, not its loads
//                  (DESIGN.md section 22). LAST: the pass writes the output image (dn_output) instead of a plane.
// A pass reads plane e[i & 1] and writes e[(i + 1) & 1]; only the last touches rgbz_out, each lane its own pixel after reading
// that pixel of rgbz_in — so rgbz_out == rgbz_in is allowed.
#include "rtu_denoise.h"

#include <vector>

namespace {

__global__ void __launch_bounds__(256) k_dn_prepare(const float4* __restrict__ rgbz, const float4* __restrict__ hits, const float4* __restrict__ albedo,
                                                    float sigma_plane, float4* __restrict__ gN, float4* __restrict__ gP, float4* __restrict__ e,
                                                    unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (i >= n) return;
    const float4 hit[3] = {hits[3 * i], hits[3 * i + 1], hits[3 * i + 2]};
    float4 n4, p4, e4;
    dn_prepare(rgbz[i], hit, albedo[i], sigma_plane, n4, p4, e4);
    gN[i] = n4;
    gP[i] = p4;
    e[i] = e4;
}

template <bool LAST>
__global__ void __launch_bounds__(256) k_dn_pass(const float4* __restrict__ gN, const float4* __restrict__ gP, const float4* __restrict__ e_in,
                                                 float4* __restrict__ e_out, const float4* rgbz_in, const float4* __restrict__ albedo, float4* rgbz_out,
                                                 int width, int height, int step, float sc2, int nlog2) {
    const int x = (int)(blockIdx.x * 32u + (threadIdx.x & 31u)), y = (int)(blockIdx.y * 8u + (threadIdx.x >> 5));
    if (x >= width || y >= height) return;
    const size_t p = (size_t)y * (size_t)width + (size_t)x;
    const bool valid = gN[p].w != 0.0f;
    float4 e = e_in[p];
    if (valid) e = dn_pass_pixel(gN, gP, e_in, width, height, x, y, step, sc2, nlog2);
    if (LAST) rgbz_out[p] = dn_output(rgbz_in[p], albedo[p], valid, e);
    else e_out[p] = e;
}

}  // namespace

int rtu_launch_denoise(const RtuDenoiseDesc& desc, const float4* rgbz_in, const float4* hits, const float4* albedo, float4* rgbz_out,
                       float4* planes, hipStream_t stream) {
    const unsigned long long n = (unsigned long long)desc.width * (unsigned long long)desc.height;
    float4* gN = planes;
    float4* gP = planes + n;
    float4* e[2] = {planes + 2 * n, planes + 3 * n};
    hipLaunchKernelGGL(k_dn_prepare, dim3((uint32_t)((n + 255ull) / 256ull)), dim3(256), 0, stream, rgbz_in, hits, albedo, desc.sigma_plane, gN, gP, e[0], n);
    const dim3 grid((uint32_t)((desc.width + 31) / 32), (uint32_t)((desc.height + 7) / 8));
    for (int i = 0; i < desc.n_passes; i++) {
        const float sc2 = dn_sc2(desc.sigma_color, i);
        if (i == desc.n_passes - 1)
            hipLaunchKernelGGL(k_dn_pass<true>, grid, dim3(256), 0, stream, gN, gP, e[i & 1], (float4*)nullptr, rgbz_in, albedo, rgbz_out, desc.width,
                               desc.height, 1 << i, sc2, desc.normal_log2_power);
        else
            hipLaunchKernelGGL(k_dn_pass<false>, grid, dim3(256), 0, stream, gN, gP, e[i & 1], e[(i + 1) & 1], (const float4*)nullptr,
                               (const float4*)nullptr, (float4*)nullptr, desc.width, desc.height, 1 << i, sc2, desc.normal_log2_power);
    }
    return (int)hipGetLastError();
}

int rtu_denoise_check_desc(const RtuDenoiseDesc* d) {
    if (!d || d->width < 1 || d->height < 1 || d->width > 65536 || d->height > 65536) return RTU_ERR_ARG;
    if (d->n_passes < 1 || d->n_passes > 8 || d->normal_log2_power < 0 || d->normal_log2_power > 7) return RTU_ERR_ARG;
    if (!(d->sigma_color > 0.0f) || !(d->sigma_plane > 0.0f)) return RTU_ERR_ARG;  // a NaN is refused too
    if (d->reserved[0] || d->reserved[1]) return RTU_ERR_ARG;
    return RTU_OK;
}

extern "C" {

int rtu_denoise_defaults(RtuDenoiseDesc* out) {
    if (!out) return RTU_ERR_ARG;
    *out = RtuDenoiseDesc{};
    out->n_passes = 5;
    out->sigma_color = 1.0f;
    out->sigma_plane = 0.05f;
    out->normal_log2_power = 5;
    return RTU_OK;
}

int rtu_denoise(const RtuDenoiseDesc* desc, const float* h_rgbz_in, const RtuRayHit* h_hits, const float* h_albedo, float* h_rgbz_out) {
    if (rtu_denoise_check_desc(desc) != RTU_OK || !h_rgbz_in || !h_hits || !h_albedo || !h_rgbz_out) return RTU_ERR_ARG;
    const int W = desc->width, H = desc->height;
    const size_t n = (size_t)W * (size_t)H;
    std::vector<float4> gN(n), gP(n), e0(n), e1(n);
    auto f4 = [](const float* p, size_t i) { return make_float4(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]); };
    for (size_t i = 0; i < n; i++) {
        const float* h = reinterpret_cast<const float*>(h_hits + i);
        const float4 hit[3] = {f4(h, 0), f4(h, 1), f4(h, 2)};
        dn_prepare(f4(h_rgbz_in, i), hit, f4(h_albedo, i), desc->sigma_plane, gN[i], gP[i], e0[i]);
    }
    std::vector<float4>* e[2] = {&e0, &e1};
    for (int i = 0; i < desc->n_passes; i++) {
        const float sc2 = dn_sc2(desc->sigma_color, i);
        const std::vector<float4>& in = *e[i & 1];
        std::vector<float4>& out = *e[(i + 1) & 1];
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const size_t p = (size_t)y * (size_t)W + (size_t)x;
                out[p] = gN[p].w != 0.0f ? dn_pass_pixel(gN.data(), gP.data(), in.data(), W, H, x, y, 1 << i, sc2, desc->normal_log2_power) : in[p];
            }
    }
    const std::vector<float4>& last = *e[desc->n_passes & 1];
    for (size_t i = 0; i < n; i++) {  // (the input pixel is read before the output pixel is written: h_rgbz_out may be h_rgbz_in)
        const float4 o = dn_output(f4(h_rgbz_in, i), f4(h_albedo, i), gN[i].w != 0.0f, last[i]);
        h_rgbz_out[4 * i] = o.x; h_rgbz_out[4 * i + 1] = o.y; h_rgbz_out[4 * i + 2] = o.z; h_rgbz_out[4 * i + 3] = o.w;
    }
    return RTU_OK;
}

}  // extern "C"
