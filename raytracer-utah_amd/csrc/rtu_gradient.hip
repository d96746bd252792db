// rtu_gradient.hip — temporal gradients of include/rtu_render.h ("Temporal gradients"): the host forms rtu_sample_luminance and
// rtu_temporal_gradient, which are the executable statement of the rules, and the kernels of the _device forms. Both call the same
// functions of rtu_gradient.h. (rtu_gradient_rays, the third host form, is in rtu_capi_temporal.hip beside rtu_extra_sample_rays; the capped
// accumulator is k_temporal<true, true, true> of rtu_temporal.hip.)
//
//   k_gradient_rays     a lane per stratum: its owner of the frame, and that pixel's ray and key of the given sample as two float4
//                       stores and two dword stores. The camera and the offsets of the sample are kernel arguments.
//   k_sample_luminance  a lane per pixel: {rgbz, first float4 of the RtuRayHit, albedo} in (48 B), one float out.
//   k_gradient_diff     a lane per stratum: its owner's guides (64 B), that node's table entry as k_temporal reads it, the one tap of
//                       the previous history (E, P, N, M and one float of the luminance plane) and the shaded gradient sample in, one
//                       float4 {num, den, noise, 0} out. A ninth of the pixels: gathers, nothing to share.
//   k_gradient_lambda   a lane per stratum: the (2 radius + 1)^2 float4 of its neighbourhood — one 16-byte load per tap, neighbouring
//                       lanes read neighbouring strata — summed in the order of the rules, one float out.
//   k_lambda_image      a lane per pixel: the lambda of its stratum.
//
// Every store is a vector store; no LDS, no atomics, no inline assembly. Nothing is read or written beyond the strata and the pixels of
// the image, whatever `owner` holds.
#include "rtu_gradient.h"

#include "rtu_intersect.h"

#include <cstring>
#include <vector>

namespace {

struct DevSinCos {
    __device__ __forceinline__ void operator()(float t, float& sn, float& cs) const { portable_sincos(t, sn, cs); }
};

__global__ void __launch_bounds__(256) k_gradient_rays(CamSample c, uint32_t frame_index, int32_t sw, uint32_t strata, float4* __restrict__ rays,
                                                       uint32_t* __restrict__ keys, uint32_t* __restrict__ owner) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= strata) return;
    int x, y;
    gr_owner(c.width, c.height, sw, s, frame_index, x, y);
    f3 org, dir;
    uint32_t key;
    camera_sample_ray(c, x, y, DevSinCos(), org, dir, key);
    rays[2 * (size_t)s] = make_float4(org.x, org.y, org.z, RTU_BIGFLOAT);
    rays[2 * (size_t)s + 1] = make_float4(dir.x, dir.y, dir.z, __uint_as_float(0u));
    keys[s] = key;
    owner[s] = (uint32_t)x + (uint32_t)c.width * (uint32_t)y;
}

__global__ void __launch_bounds__(256) k_sample_luminance(unsigned long long pixels, const float4* __restrict__ rgbz, const float4* __restrict__ hits,
                                                          const float4* __restrict__ albedo, float* __restrict__ lum) {
    const unsigned long long p = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (p >= pixels) return;
    lum[p] = gr_luminance(rgbz[p], hits[3 * p], albedo[p]);
}

__global__ void __launch_bounds__(256) k_gradient_diff(GrParams G, const float4* __restrict__ hits, const float4* __restrict__ albedo,
                                                       const RtuNodeMotion* __restrict__ motion, const float4* __restrict__ hist_prev,
                                                       const float* __restrict__ lum_prev, const uint32_t* __restrict__ owner,
                                                       const float4* __restrict__ rgbt, float4* __restrict__ diff) {
    const TpParams& P = G.M.P;
    const uint32_t strata = (uint32_t)G.sw * (uint32_t)G.sh;
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= strata) return;
    const size_t n = (size_t)P.width * (size_t)P.height;
    const size_t p = owner[s];
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (p < n) {
        const int y = (int)(p / (size_t)P.width), x = (int)(p - (size_t)y * (size_t)P.width);
        const float4 hit[3] = {hits[3 * p], hits[3 * p + 1], hits[3 * p + 2]};
        const int32_t k = tp_motion_index(hit[0], G.M.n_nodes);
        const TpMotion T = tp_load_motion(motion, k);
        const float4* h[4];
        for (int i = 0; i < 4; i++) h[i] = hist_prev ? hist_prev + i * n : nullptr;
        g = gr_diff(G.M, k >= 0, T, h, lum_prev, x, y, hit, albedo[p], rgbt[s]);
    }
    diff[s] = g;
}

__global__ void __launch_bounds__(256) k_gradient_lambda(GrParams G, const float4* __restrict__ diff, float* __restrict__ lambda) {
    const int sx = (int)(blockIdx.x * 32u + (threadIdx.x & 31u)), sy = (int)(blockIdx.y * 8u + (threadIdx.x >> 5));
    if (sx >= G.sw || sy >= G.sh) return;
    lambda[(size_t)sy * (size_t)G.sw + (size_t)sx] = gr_lambda(G, diff, sx, sy);
}

__global__ void __launch_bounds__(256) k_lambda_image(int32_t width, int32_t height, int32_t sw, const float* __restrict__ lambda, float* __restrict__ out) {
    const int x = (int)(blockIdx.x * 32u + (threadIdx.x & 31u)), y = (int)(blockIdx.y * 8u + (threadIdx.x >> 5));
    if (x >= width || y >= height) return;
    out[(size_t)y * (size_t)width + (size_t)x] = lambda ? lambda[(size_t)(y / TP_STRATUM) * (size_t)sw + (size_t)(x / TP_STRATUM)] : 0.0f;
}

// the host form's table entry (a table of any alignment)
TpMotion host_entry(const RtuNodeMotion* motion, int32_t k) {
    TpMotion T = tp_motion_identity();
    if (k >= 0) {
        memcpy(T.m, motion[k].m, sizeof T.m);
        memcpy(T.g, motion[k].g, sizeof T.g);
        T.flags = motion[k].flags;
    }
    return T;
}

}  // namespace

int rtu_launch_gradient_rays(const CamSample& c, uint32_t frame_index, float4* rays, uint32_t* keys, uint32_t* owner, hipStream_t stream) {
    const int32_t sw = gr_strata(c.width), sh = gr_strata(c.height);
    const uint32_t strata = (uint32_t)sw * (uint32_t)sh;
    if (strata == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_gradient_rays, dim3((strata + 255u) / 256u), dim3(256), 0, stream, c, frame_index, sw, strata, rays, keys, owner);
    return (int)hipGetLastError();
}

int rtu_launch_sample_luminance(size_t pixels, const float4* rgbz, const float4* hits, const float4* albedo, float* lum, hipStream_t stream) {
    if (pixels == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_sample_luminance, dim3((uint32_t)((pixels + 255) / 256)), dim3(256), 0, stream, (unsigned long long)pixels, rgbz, hits, albedo, lum);
    return (int)hipGetLastError();
}

int rtu_launch_temporal_gradient(const GrParams& g, const float4* hits, const float4* albedo, const RtuNodeMotion* d_motion, const float4* hist_prev,
                                 const float* lum_prev, const uint32_t* owner, const float4* rgbt, float4* diff, float* lambda, hipStream_t stream) {
    const uint32_t strata = (uint32_t)g.sw * (uint32_t)g.sh;
    hipLaunchKernelGGL(k_gradient_diff, dim3((strata + 255u) / 256u), dim3(256), 0, stream, g, hits, albedo, d_motion, hist_prev, lum_prev, owner, rgbt, diff);
    hipLaunchKernelGGL(k_gradient_lambda, dim3((uint32_t)((g.sw + 31) / 32), (uint32_t)((g.sh + 7) / 8)), dim3(256), 0, stream, g, diff, lambda);
    return (int)hipGetLastError();
}

int rtu_launch_lambda_image(int32_t width, int32_t height, const float* lambda, float* out, hipStream_t stream) {
    const dim3 grid((uint32_t)((width + 31) / 32), (uint32_t)((height + 7) / 8));
    hipLaunchKernelGGL(k_lambda_image, grid, dim3(256), 0, stream, width, height, gr_strata(width), lambda, out);
    return (int)hipGetLastError();
}

int rtu_gradient_check_desc(const RtuGradientDesc* d) {
    if (!d || d->width < 1 || d->height < 1 || d->width > 65536 || d->height > 65536) return RTU_ERR_ARG;
    if ((unsigned long long)d->width * (unsigned long long)d->height > (1ull << 26)) return RTU_ERR_ARG;
    if (d->radius < 0 || d->radius > GR_MAX_RADIUS || !(d->kappa >= 0.0f) || !tp_finite(d->kappa) || d->enabled > 1u) return RTU_ERR_ARG;  // a NaN is refused too
    if (d->reserved[0] || d->reserved[1]) return RTU_ERR_ARG;
    return RTU_OK;
}

extern "C" {

int rtu_gradient_defaults(RtuGradientDesc* out) {
    if (!out) return RTU_ERR_ARG;
    *out = RtuGradientDesc{};
    out->radius = 1;
    out->kappa = 2.0f;
    out->enabled = 1;
    return RTU_OK;
}

int rtu_sample_luminance(const RtuGradientDesc* desc, const float* h_rgbz, const RtuRayHit* h_hits, const float* h_albedo, float* h_lum) {
    if (rtu_gradient_check_desc(desc) != RTU_OK || !h_rgbz || !h_hits || !h_albedo || !h_lum) return RTU_ERR_ARG;
    const size_t n = (size_t)desc->width * (size_t)desc->height;
    const float* h = reinterpret_cast<const float*>(h_hits);
    for (size_t p = 0; p < n; p++) h_lum[p] = gr_luminance(f4(h_rgbz, p), f4(h, 3 * p), f4(h_albedo, p));
    return RTU_OK;
}

int rtu_temporal_gradient(const RtuTemporalDesc* desc, const RtuGradientDesc* gdesc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam,
                          const RtuRayHit* h_hits, const float* h_albedo, const RtuNodeMotion* motion, uint32_t n_nodes, const float* h_hist_prev,
                          const float* h_lum_prev, const uint32_t* owner, const float* h_rgbt, float* h_diff_out, float* h_lambda_out) {
    if (rtu_temporal_check_desc(desc) != RTU_OK || rtu_gradient_check_desc(gdesc) != RTU_OK || gdesc->width != desc->width || gdesc->height != desc->height)
        return RTU_ERR_ARG;
    if (!cur_cam || !h_hits || !h_albedo || !motion || !owner || !h_rgbt || !h_diff_out || !h_lambda_out) return RTU_ERR_ARG;
    if (rtu_temporal_check_motion(motion, n_nodes, 0) != RTU_OK) return RTU_ERR_ARG;
    if (h_hist_prev && (!prev_cam || !h_lum_prev)) return RTU_ERR_ARG;
    if (!prev_cam) prev_cam = cur_cam;
    if (cur_cam->width != desc->width || cur_cam->height != desc->height || prev_cam->width != desc->width || prev_cam->height != desc->height)
        return RTU_ERR_ARG;
    const int W = desc->width;
    const size_t n = (size_t)W * (size_t)desc->height;
    GrParams G{};
    G.M = tp_motion_setup(*desc, *prev_cam, *cur_cam, h_hist_prev != nullptr, n_nodes, 0);
    G.sw = gr_strata(desc->width);
    G.sh = gr_strata(desc->height);
    G.radius = gdesc->radius;
    G.kappa = gdesc->kappa;
    const size_t strata = (size_t)G.sw * (size_t)G.sh;
    for (size_t s = 0; s < strata; s++)
        if ((size_t)owner[s] >= n) return RTU_ERR_ARG;
    std::vector<float4> prev;  // (the planes as float4: the caller's floats need not be 16-byte aligned)
    const float4* hp[4] = {};
    if (h_hist_prev) {
        prev.resize(4 * n);
        for (size_t i = 0; i < 4 * n; i++) prev[i] = f4(h_hist_prev, i);
        for (int i = 0; i < 4; i++) hp[i] = prev.data() + i * n;
    }
    std::vector<float4> diff(strata);
    for (size_t s = 0; s < strata; s++) {
        const size_t p = owner[s];
        const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * (size_t)W);
        const float* h = reinterpret_cast<const float*>(h_hits + p);
        const float4 hit[3] = {f4(h, 0), f4(h, 1), f4(h, 2)};
        const int32_t k = tp_motion_index(hit[0], n_nodes);
        diff[s] = gr_diff(G.M, k >= 0, host_entry(motion, k), hp, h_lum_prev, x, y, hit, f4(h_albedo, p), f4(h_rgbt, s));
        st4(h_diff_out, s, diff[s]);
    }
    for (int sy = 0; sy < G.sh; sy++)
        for (int sx = 0; sx < G.sw; sx++) h_lambda_out[(size_t)sy * (size_t)G.sw + (size_t)sx] = gr_lambda(G, diff.data(), sx, sy);
    return RTU_OK;
}

}  // extern "C"
