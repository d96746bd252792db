// rtu_temporal.hip — the temporal accumulator of include/rtu_render.h ("Temporal accumulation", "... across scene updates", and the
// moments of "Variance-guided filtering"): its host forms rtu_temporal_accumulate, _motion and _moments, which are the executable
// statement of the rules, and the kernels of their _device forms. Both call tp_pixel<MOVING, MOMENTS> of rtu_temporal.h, pixel by
// pixel; the three forms are the instantiations <false, false>, <true, false> and <true, true> of one kernel and of one host loop,
// rtu_temporal_accumulate_gradient ("Temporal gradients") is <true, true, true> and rtu_temporal_accumulate_sparse ("Sparse
// sessions") is <true, true, false, true>.
//
//   k_temporal          one lane per pixel, 32 x 8 pixel workgroups as k_dn_pass (a wavefront is two rows of 32). A lane reads its
//                       pixel's {rgbz, RtuRayHit, albedo} (80 B), up to four taps of the previous history — three 16-byte loads each,
//                       neighbouring lanes' taps are neighbouring pixels while the surface is smooth, so the lines are shared through
//                       the vector L1 —, and writes its pixel of the image and of the three planes of the new history (64 B). No
//                       LDS, no atomics. Without MOVING the lookup mode is wave-uniform (a kernel argument, TpParams).
//     MOVING            a moving scene (TpMotionParams): besides, a lane reads the table entry of its pixel's node, 96 B as six
//                       16-byte loads STRAIGHT FROM GLOBAL MEMORY: the table has no bound that LDS could hold, the lanes of a
//                       wavefront mostly show one or two nodes — lanes with one address are served by one request — and the few
//                       entries a frame touches stay in the vector L1. The lookup mode (none, one tap, four taps) is per lane;
//                       single exit, select on values.
//     MOMENTS           a four-plane history: besides, one 16-byte load of M per ACCEPTED tap and one 16-byte store.
//     GRADIENT          besides, one dword load of the lambda of the pixel's stratum: the three lanes of a stratum's row share it.
//     SPARSE            in place of the 16-byte load of rgbz one dword load of the owner of the pixel's block — the lanes of a block's
//                       row share it — and, in the one lane of a block that is the owner, the 16-byte load of the block's sample;
//                       besides, one byte store of the pixel's mark in the hole plane.
//   k_temporal_sensor   <MODEL, MOMENTS> ("Temporal accumulation for sensors"): k_temporal without MOVING whose lookup goes through the
//                       projection of a panoramic, fisheye or orthographic sensor (sensor_project of rtu_sensor.h: a few binary32
//                       operations and one or two binary64 acos per pixel) in place of the pinhole's; the previous RtuSensorDesc is a
//                       kernel argument, the model a template parameter. A panorama's tap columns wrap at the seam. Its host forms
//                       are rtu_temporal_accumulate_sensor and _sensor_moments.
//   k_temporal_deform   <MOMENTS> ("Temporal accumulation on deforming meshes"): k_temporal<true, MOMENTS> whose lanes also read their pixel's
//                       surface record (32 B, two 16-byte loads) and, where the node's entry is RTU_MOTION_DEFORM, the node's mesh id, the
//                       mesh's header, six indices and six vectors of the PREVIOUS vertices and normals — plain global loads, per lane
//                       (neighbouring pixels show neighbouring faces) — and carry that point through the entry in place of the hit's.
//                       Every other pixel is the motion form's, bit for bit. k_motion_vectors_deform likewise.
//   k_temporal_history  one lane per pixel: the history length out of the E plane.
//   k_motion_vectors    one lane per pixel: its RtuRayHit and its node's entry in, one float4 out.
// Each lane reads its pixel of rgbz before it writes that pixel of rgbz_out and touches no other: rgbz_out == rgbz is allowed. Taps read
// anywhere in hist_prev: hist_out must not overlap it.
#include "rtu_temporal.h"

#include <cstring>
#include <vector>

namespace {

// `motion` is read with MOVING only; hist_prev and hist_out have three planes, with MOMENTS four
template <bool MOVING, bool MOMENTS, bool GRADIENT = false, bool SPARSE = false>
__global__ void __launch_bounds__(256) k_temporal(TpArgs<MOVING, GRADIENT, SPARSE> A, const float4* rgbz, const float4* __restrict__ hits, const float4* __restrict__ albedo,
                                                  const float4* __restrict__ hist_prev, float4* __restrict__ hist_out, float4* rgbz_out,
                                                  const RtuNodeMotion* __restrict__ motion) {
    constexpr int PLANES = MOMENTS ? 4 : 3;
    const TpParams& P = tp_base(A);
    const int x = (int)(blockIdx.x * 32u + (threadIdx.x & 31u)), y = (int)(blockIdx.y * 8u + (threadIdx.x >> 5));
    if (x >= P.width || y >= P.height) return;
    const size_t n = (size_t)P.width * (size_t)P.height;
    const size_t p = (size_t)y * (size_t)P.width + (size_t)x;
    const float4 hit[3] = {hits[3 * p], hits[3 * p + 1], hits[3 * p + 2]};
    int32_t k = -1;
    if constexpr (MOVING) k = tp_motion_index(hit[0], tp_motion(A).n_nodes);
    const TpMotion T = tp_load_motion(motion, k);
    const float4* h[PLANES];
    for (int i = 0; i < PLANES; i++) h[i] = hist_prev ? hist_prev + i * n : nullptr;
    float4 out, o[PLANES];
    if constexpr (SPARSE) {  // (rgbz is not read) the sample of the pixel's block where the pixel owns it
        const size_t b = (size_t)((uint32_t)y / (uint32_t)A.block) * (size_t)A.sw + (size_t)((uint32_t)x / (uint32_t)A.block);
        const bool own = (size_t)A.owner[b] == p;
        const float4 in = own ? A.rgbt[b] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        uint8_t hole;
        tp_pixel<MOVING, MOMENTS, GRADIENT, SPARSE>(A, k >= 0, T, h, x, y, in, hit, albedo[p], out, o, own, &hole);
        A.hole[p] = hole;
    } else {
        tp_pixel<MOVING, MOMENTS, GRADIENT>(A, k >= 0, T, h, x, y, rgbz[p], hit, albedo[p], out, o);
    }
    rgbz_out[p] = out;
    for (int i = 0; i < PLANES; i++) hist_out[i * n + p] = o[i];
}

template <bool MOMENTS>
__global__ void __launch_bounds__(256) k_temporal_deform(TpMotionParams A, TpDeformScene D, const float4* rgbz, const float4* __restrict__ hits,
                                                         const float4* __restrict__ albedo, const float4* __restrict__ surface,
                                                         const float4* __restrict__ hist_prev, float4* __restrict__ hist_out, float4* rgbz_out,
                                                         const RtuNodeMotion* __restrict__ motion) {
    constexpr int PLANES = MOMENTS ? 4 : 3;
    const TpParams& P = A.P;
    const int x = (int)(blockIdx.x * 32u + (threadIdx.x & 31u)), y = (int)(blockIdx.y * 8u + (threadIdx.x >> 5));
    if (x >= P.width || y >= P.height) return;
    const size_t n = (size_t)P.width * (size_t)P.height;
    const size_t p = (size_t)y * (size_t)P.width + (size_t)x;
    const float4 hit[3] = {hits[3 * p], hits[3 * p + 1], hits[3 * p + 2]};
    const int32_t k = tp_motion_index(hit[0], A.n_nodes);
    TpMotion T = tp_load_motion(motion, k);
    f3 src[2];
    const bool ok = tp_deform_source(D, k, T, surface[2 * p], surface[2 * p + 1], mk3(hit[1].x, hit[1].y, hit[1].z), mk3(hit[2].x, hit[2].y, hit[2].z), src[0],
                                     src[1]);
    const float4* h[PLANES];
    for (int i = 0; i < PLANES; i++) h[i] = hist_prev ? hist_prev + i * n : nullptr;
    float4 out, o[PLANES];
    tp_pixel<true, MOMENTS, false, false, TpPinhole, true>(A, k >= 0, T, h, x, y, rgbz[p], hit, albedo[p], out, o, true, nullptr, TpPinhole(), src, ok);
    rgbz_out[p] = out;
    for (int i = 0; i < PLANES; i++) hist_out[i * n + p] = o[i];
}

template <bool MOVING, bool MOMENTS, bool GRADIENT = false, bool SPARSE = false>
int launch_temporal(const TpArgs<MOVING, GRADIENT, SPARSE>& a, const float4* rgbz, const float4* hits, const float4* albedo, const float4* hist_prev, float4* hist_out,
                    float4* rgbz_out, const RtuNodeMotion* d_motion, hipStream_t stream) {
    const dim3 grid((uint32_t)((tp_base(a).width + 31) / 32), (uint32_t)((tp_base(a).height + 7) / 8));
    hipLaunchKernelGGL((k_temporal<MOVING, MOMENTS, GRADIENT, SPARSE>), grid, dim3(256), 0, stream, a, rgbz, hits, albedo, hist_prev, hist_out, rgbz_out, d_motion);
    return (int)hipGetLastError();
}

// The sensor forms: k_temporal<false, MOMENTS> with the projection of sensor model MODEL in place of the pinhole's. `prev`, the
// previous sensor, is a kernel argument (scalar loads); the model is a template parameter, no lane branches on it.
template <int MODEL, bool MOMENTS>
__global__ void __launch_bounds__(256) k_temporal_sensor(TpParams P, RtuSensorDesc prev, const float4* rgbz, const float4* __restrict__ hits,
                                                         const float4* __restrict__ albedo, const float4* __restrict__ hist_prev,
                                                         float4* __restrict__ hist_out, float4* rgbz_out) {
    constexpr int PLANES = MOMENTS ? 4 : 3;
    const int x = (int)(blockIdx.x * 32u + (threadIdx.x & 31u)), y = (int)(blockIdx.y * 8u + (threadIdx.x >> 5));
    if (x >= P.width || y >= P.height) return;
    const size_t n = (size_t)P.width * (size_t)P.height;
    const size_t p = (size_t)y * (size_t)P.width + (size_t)x;
    const float4 hit[3] = {hits[3 * p], hits[3 * p + 1], hits[3 * p + 2]};
    const float4* h[PLANES];
    for (int i = 0; i < PLANES; i++) h[i] = hist_prev ? hist_prev + i * n : nullptr;
    float4 out, o[PLANES];
    tp_pixel<false, MOMENTS, false, false, TpSensorProj<MODEL>>(P, false, tp_motion_identity(), h, x, y, rgbz[p], hit, albedo[p], out, o, true, nullptr,
                                                                TpSensorProj<MODEL>{prev});
    rgbz_out[p] = out;
    for (int i = 0; i < PLANES; i++) hist_out[i * n + p] = o[i];
}

template <int MODEL>
int launch_temporal_sensor(const TpParams& p, const RtuSensorDesc& prev, bool moments, const float4* rgbz, const float4* hits, const float4* albedo,
                           const float4* hist_prev, float4* hist_out, float4* rgbz_out, hipStream_t stream) {
    const dim3 grid((uint32_t)((p.width + 31) / 32), (uint32_t)((p.height + 7) / 8));
    if (moments) hipLaunchKernelGGL((k_temporal_sensor<MODEL, true>), grid, dim3(256), 0, stream, p, prev, rgbz, hits, albedo, hist_prev, hist_out, rgbz_out);
    else hipLaunchKernelGGL((k_temporal_sensor<MODEL, false>), grid, dim3(256), 0, stream, p, prev, rgbz, hits, albedo, hist_prev, hist_out, rgbz_out);
    return (int)hipGetLastError();
}

__global__ void __launch_bounds__(256) k_motion_vectors(TpParams P, uint32_t n_nodes, const float4* __restrict__ hits,
                                                        const RtuNodeMotion* __restrict__ motion, float4* __restrict__ mv) {
    const int x = (int)(blockIdx.x * 32u + (threadIdx.x & 31u)), y = (int)(blockIdx.y * 8u + (threadIdx.x >> 5));
    if (x >= P.width || y >= P.height) return;
    const size_t p = (size_t)y * (size_t)P.width + (size_t)x;
    const float4 hit[3] = {hits[3 * p], hits[3 * p + 1], hits[3 * p + 2]};
    const int32_t k = tp_motion_index(hit[0], n_nodes);
    mv[p] = tp_motion_vector(P, k >= 0, tp_load_motion(motion, k), hit);
}

__global__ void __launch_bounds__(256) k_motion_vectors_deform(TpParams P, uint32_t n_nodes, TpDeformScene D, const float4* __restrict__ hits,
                                                               const float4* __restrict__ surface, const RtuNodeMotion* __restrict__ motion,
                                                               float4* __restrict__ mv) {
    const int x = (int)(blockIdx.x * 32u + (threadIdx.x & 31u)), y = (int)(blockIdx.y * 8u + (threadIdx.x >> 5));
    if (x >= P.width || y >= P.height) return;
    const size_t p = (size_t)y * (size_t)P.width + (size_t)x;
    const float4 hit[3] = {hits[3 * p], hits[3 * p + 1], hits[3 * p + 2]};
    const int32_t k = tp_motion_index(hit[0], n_nodes);
    TpMotion T = tp_load_motion(motion, k);
    f3 src[2];
    const bool ok = tp_deform_source(D, k, T, surface[2 * p], surface[2 * p + 1], mk3(hit[1].x, hit[1].y, hit[1].z), mk3(hit[2].x, hit[2].y, hit[2].z), src[0],
                                     src[1]);
    mv[p] = tp_motion_vector_deform(P, k >= 0, T, src, ok);
}

__global__ void __launch_bounds__(256) k_temporal_history(const float4* __restrict__ hist, float* __restrict__ n_out, unsigned long long pixels) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (i >= pixels) return;
    n_out[i] = hist ? hist[i].w : 0.0f;
}

}  // namespace

int rtu_launch_temporal(const TpParams& p, const float4* rgbz, const float4* hits, const float4* albedo, const float4* hist_prev, float4* hist_out,
                        float4* rgbz_out, hipStream_t stream) {
    return launch_temporal<false, false>(p, rgbz, hits, albedo, hist_prev, hist_out, rgbz_out, nullptr, stream);
}

int rtu_launch_temporal_motion(const TpMotionParams& m, const float4* rgbz, const float4* hits, const float4* albedo, const float4* hist_prev,
                               float4* hist_out, float4* rgbz_out, const RtuNodeMotion* d_motion, hipStream_t stream) {
    return launch_temporal<true, false>(m, rgbz, hits, albedo, hist_prev, hist_out, rgbz_out, d_motion, stream);
}

int rtu_launch_temporal_moments(const TpMotionParams& m, const float4* rgbz, const float4* hits, const float4* albedo, const float4* hist_prev,
                                float4* hist_out, float4* rgbz_out, const RtuNodeMotion* d_motion, hipStream_t stream) {
    return launch_temporal<true, true>(m, rgbz, hits, albedo, hist_prev, hist_out, rgbz_out, d_motion, stream);
}

int rtu_launch_temporal_deform(const TpMotionParams& m, bool moments, const TpDeformScene& D, const float4* rgbz, const float4* hits, const float4* albedo,
                               const float4* surface, const float4* hist_prev, float4* hist_out, float4* rgbz_out, const RtuNodeMotion* d_motion,
                               hipStream_t stream) {
    const dim3 grid((uint32_t)((m.P.width + 31) / 32), (uint32_t)((m.P.height + 7) / 8));
    if (moments)
        hipLaunchKernelGGL((k_temporal_deform<true>), grid, dim3(256), 0, stream, m, D, rgbz, hits, albedo, surface, hist_prev, hist_out, rgbz_out, d_motion);
    else hipLaunchKernelGGL((k_temporal_deform<false>), grid, dim3(256), 0, stream, m, D, rgbz, hits, albedo, surface, hist_prev, hist_out, rgbz_out, d_motion);
    return (int)hipGetLastError();
}

int rtu_launch_motion_vectors_deform(const TpParams& p, uint32_t n_nodes, const TpDeformScene& D, const float4* hits, const float4* surface,
                                     const RtuNodeMotion* d_motion, float4* mv, hipStream_t stream) {
    const dim3 grid((uint32_t)((p.width + 31) / 32), (uint32_t)((p.height + 7) / 8));
    hipLaunchKernelGGL(k_motion_vectors_deform, grid, dim3(256), 0, stream, p, n_nodes, D, hits, surface, d_motion, mv);
    return (int)hipGetLastError();
}

int rtu_launch_temporal_capped(const TpGradientParams& g, const float4* rgbz, const float4* hits, const float4* albedo, const float4* hist_prev,
                               float4* hist_out, float4* rgbz_out, const RtuNodeMotion* d_motion, hipStream_t stream) {
    return launch_temporal<true, true, true>(g, rgbz, hits, albedo, hist_prev, hist_out, rgbz_out, d_motion, stream);
}

int rtu_launch_temporal_sparse(const TpSparseParams& s, const float4* hits, const float4* albedo, const float4* hist_prev, float4* hist_out,
                               float4* rgbz_out, const RtuNodeMotion* d_motion, hipStream_t stream) {
    return launch_temporal<true, true, false, true>(s, nullptr, hits, albedo, hist_prev, hist_out, rgbz_out, d_motion, stream);
}

int rtu_launch_temporal_sensor(const TpParams& p, const RtuSensorDesc& prev, bool moments, const float4* rgbz, const float4* hits, const float4* albedo,
                               const float4* hist_prev, float4* hist_out, float4* rgbz_out, hipStream_t stream) {
    switch (prev.model) {
    case RTU_SENSOR_EQUIRECT: return launch_temporal_sensor<RTU_SENSOR_EQUIRECT>(p, prev, moments, rgbz, hits, albedo, hist_prev, hist_out, rgbz_out, stream);
    case RTU_SENSOR_FISHEYE: return launch_temporal_sensor<RTU_SENSOR_FISHEYE>(p, prev, moments, rgbz, hits, albedo, hist_prev, hist_out, rgbz_out, stream);
    default: return launch_temporal_sensor<RTU_SENSOR_ORTHO>(p, prev, moments, rgbz, hits, albedo, hist_prev, hist_out, rgbz_out, stream);
    }
}

int rtu_launch_temporal_history(const float4* hist, float* n_out, size_t pixels, hipStream_t stream) {
    if (pixels == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_temporal_history, dim3((uint32_t)((pixels + 255) / 256)), dim3(256), 0, stream, hist, n_out, (unsigned long long)pixels);
    return (int)hipGetLastError();
}

int rtu_launch_motion_vectors(const TpParams& p, uint32_t n_nodes, const float4* hits, const RtuNodeMotion* d_motion, float4* mv, hipStream_t stream) {
    const dim3 grid((uint32_t)((p.width + 31) / 32), (uint32_t)((p.height + 7) / 8));
    hipLaunchKernelGGL(k_motion_vectors, grid, dim3(256), 0, stream, p, n_nodes, hits, d_motion, mv);
    return (int)hipGetLastError();
}

int rtu_temporal_check_motion(const RtuNodeMotion* h, uint32_t n_nodes, int32_t history_cap, bool allow_deform) {
    if (history_cap < 0 || history_cap > 65535) return RTU_ERR_ARG;
    const uint32_t known = RTU_MOTION_STATIC | RTU_MOTION_RESET | (allow_deform ? RTU_MOTION_DEFORM : 0u);
    if (h)
        for (uint32_t i = 0; i < n_nodes; i++)
            if ((h[i].flags & ~known) || h[i].reserved[0] || h[i].reserved[1]) return RTU_ERR_ARG;
    return RTU_OK;
}

static TpMotion host_motion(const RtuNodeMotion* motion, int32_t k) {
    TpMotion T = tp_motion_identity();
    if (k >= 0) {
        memcpy(T.m, motion[k].m, sizeof T.m);
        memcpy(T.g, motion[k].g, sizeof T.g);
        T.flags = motion[k].flags;
    }
    return T;
}

int rtu_temporal_check_desc(const RtuTemporalDesc* d) {
    if (!d || d->width < 1 || d->height < 1 || d->width > 65536 || d->height > 65536) return RTU_ERR_ARG;
    if ((unsigned long long)d->width * (unsigned long long)d->height > (1ull << 26)) return RTU_ERR_ARG;
    if (d->max_history < 1 || d->max_history > 65535) return RTU_ERR_ARG;
    if (!(d->sigma_plane > 0.0f) || !(d->normal_min >= -1.0f && d->normal_min <= 1.0f)) return RTU_ERR_ARG;  // a NaN is refused too
    if (d->flags & ~RTU_TEMPORAL_DENOISE) return RTU_ERR_ARG;
    if (d->reserved[0] || d->reserved[1]) return RTU_ERR_ARG;
    return RTU_OK;
}

// what the sparse host form has in place of h_rgbz: one sample and one owner per block, and the hole plane it writes
struct SparseHost {
    const RtuSparseDesc* desc;
    const float*         rgbt;
    const uint32_t*      owner;
    uint8_t*             hole;
};

// the host forms: motion, n_nodes and history_cap are read with MOVING only; the histories have three planes, with MOMENTS four;
// lambda (one float per stratum, or nullptr) is read with GRADIENT only; sp with SPARSE only, and then h_rgbz is not read
template <bool MOVING, bool MOMENTS, bool GRADIENT = false, bool SPARSE = false>
static int accumulate_host(const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam, const float* h_rgbz, const RtuRayHit* h_hits,
                           const float* h_albedo, const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out, const RtuNodeMotion* motion,
                           uint32_t n_nodes, int32_t history_cap, const float* lambda = nullptr, const SparseHost* sp = nullptr) {
    constexpr int PLANES = MOMENTS ? 4 : 3;
    if (rtu_temporal_check_desc(desc) != RTU_OK || !cur_cam || (!SPARSE && !h_rgbz) || !h_hits || !h_albedo || !h_hist_out || !h_rgbz_out) return RTU_ERR_ARG;
    if constexpr (SPARSE)
        if (rtu_sparse_check_desc(sp->desc) != RTU_OK || sp->desc->width != desc->width || sp->desc->height != desc->height || !sp->rgbt || !sp->owner || !sp->hole)
            return RTU_ERR_ARG;
    if (MOVING && (!motion || rtu_temporal_check_motion(motion, n_nodes, history_cap) != RTU_OK)) return RTU_ERR_ARG;
    if (h_hist_prev && !prev_cam) return RTU_ERR_ARG;
    if (!prev_cam) prev_cam = cur_cam;
    if (cur_cam->width != desc->width || cur_cam->height != desc->height || prev_cam->width != desc->width || prev_cam->height != desc->height)
        return RTU_ERR_ARG;
    const int W = desc->width, H = desc->height;
    const size_t n = (size_t)W * (size_t)H;
    if (h_hist_prev) {  // taps read anywhere in the previous history
        const uintptr_t a = (uintptr_t)h_hist_prev, b = (uintptr_t)h_hist_out, bytes = 16 * PLANES * n;
        if (a < b + bytes && b < a + bytes) return RTU_ERR_ARG;
    }
    TpArgs<MOVING, GRADIENT, SPARSE> A;
    if constexpr (SPARSE) A = TpSparseParams{tp_motion_setup(*desc, *prev_cam, *cur_cam, h_hist_prev != nullptr, n_nodes, history_cap), nullptr, nullptr, nullptr,
                                             sp->desc->block, (W + sp->desc->block - 1) / sp->desc->block};
    else if constexpr (GRADIENT) A = TpGradientParams{tp_motion_setup(*desc, *prev_cam, *cur_cam, h_hist_prev != nullptr, n_nodes, history_cap), lambda,
                                                 (W + TP_STRATUM - 1) / TP_STRATUM};
    else if constexpr (MOVING) A = tp_motion_setup(*desc, *prev_cam, *cur_cam, h_hist_prev != nullptr, n_nodes, history_cap);
    else A = tp_setup(*desc, *prev_cam, *cur_cam, h_hist_prev != nullptr);
    std::vector<float4> prev;  // (the planes as float4: the caller's floats need not be 16-byte aligned)
    const float4* hp[PLANES] = {};
    if (h_hist_prev) {
        prev.resize(PLANES * n);
        for (size_t i = 0; i < PLANES * n; i++) prev[i] = f4(h_hist_prev, i);
        for (int i = 0; i < PLANES; i++) hp[i] = prev.data() + i * n;
    }
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * (size_t)W + (size_t)x;
            const float* h = reinterpret_cast<const float*>(h_hits + p);
            const float4 hit[3] = {f4(h, 0), f4(h, 1), f4(h, 2)};
            const int32_t k = MOVING ? tp_motion_index(hit[0], n_nodes) : -1;
            float4 out, o[PLANES];
            if constexpr (SPARSE) {
                const size_t b = (size_t)(y / A.block) * (size_t)A.sw + (size_t)(x / A.block);
                const bool own = (size_t)sp->owner[b] == p;
                const float4 in = own ? f4(sp->rgbt, b) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                tp_pixel<MOVING, MOMENTS, GRADIENT, SPARSE>(A, k >= 0, host_motion(motion, k), hp, x, y, in, hit, f4(h_albedo, p), out, o, own, sp->hole + p);
            } else {
                tp_pixel<MOVING, MOMENTS, GRADIENT>(A, k >= 0, host_motion(motion, k), hp, x, y, f4(h_rgbz, p), hit, f4(h_albedo, p), out, o);
            }
            st4(h_rgbz_out, p, out);  // (the input pixel was read before: h_rgbz_out may be h_rgbz)
            for (int i = 0; i < PLANES; i++) st4(h_hist_out, i * n + p, o[i]);
        }
    return RTU_OK;
}

// The host forms of the deform accumulators: accumulate_host<true, MOMENTS> with the surface records, and the previous vertices and
// the connectivity read from the PREVIOUS scene.
struct DeformHost {
    std::vector<TpDeformMesh> meshes;
    std::vector<int32_t>      node_mesh;
    TpDeformScene             D;
};
static bool deform_host_setup(const RtuSceneDesc* prev, uint32_t n_nodes, DeformHost& dh) {
    if (!prev || prev->n_nodes != n_nodes || (prev->n_nodes && !prev->nodes) || (prev->n_meshes && !prev->meshes)) return false;
    dh.meshes.resize(prev->n_meshes);
    for (uint32_t i = 0; i < prev->n_meshes; i++) {
        const RtuMesh& m = prev->meshes[i];
        // (a mesh without one of its arrays has no face to look up: nf = 0, every record on it is out of range)
        dh.meshes[i] = TpDeformMesh{m.f, m.fn, m.v, m.vn, (m.f && m.fn && m.v && m.vn) ? m.nf : 0u, 0};
    }
    dh.node_mesh.resize(n_nodes);
    for (uint32_t i = 0; i < n_nodes; i++) dh.node_mesh[i] = prev->nodes[i].mesh_id;
    dh.D = TpDeformScene{dh.meshes.data(), dh.node_mesh.data(), prev->n_meshes, 0};
    return true;
}

template <bool MOMENTS>
static int accumulate_deform_host(const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam, const float* h_rgbz,
                                  const RtuRayHit* h_hits, const float* h_albedo, const RtuRaySurface* h_surface, const RtuSceneDesc* prev_scene,
                                  const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out, const RtuNodeMotion* motion, uint32_t n_nodes,
                                  int32_t history_cap) {
    constexpr int PLANES = MOMENTS ? 4 : 3;
    if (rtu_temporal_check_desc(desc) != RTU_OK || !cur_cam || !h_rgbz || !h_hits || !h_albedo || !h_surface || !h_hist_out || !h_rgbz_out) return RTU_ERR_ARG;
    if (!motion || rtu_temporal_check_motion(motion, n_nodes, history_cap, true) != RTU_OK) return RTU_ERR_ARG;
    DeformHost dh;
    if (!deform_host_setup(prev_scene, n_nodes, dh)) return RTU_ERR_ARG;
    if (h_hist_prev && !prev_cam) return RTU_ERR_ARG;
    if (!prev_cam) prev_cam = cur_cam;
    if (cur_cam->width != desc->width || cur_cam->height != desc->height || prev_cam->width != desc->width || prev_cam->height != desc->height)
        return RTU_ERR_ARG;
    const int W = desc->width, H = desc->height;
    const size_t n = (size_t)W * (size_t)H;
    if (h_hist_prev) {  // taps read anywhere in the previous history
        const uintptr_t a = (uintptr_t)h_hist_prev, b = (uintptr_t)h_hist_out, bytes = 16 * PLANES * n;
        if (a < b + bytes && b < a + bytes) return RTU_ERR_ARG;
    }
    const TpMotionParams A = tp_motion_setup(*desc, *prev_cam, *cur_cam, h_hist_prev != nullptr, n_nodes, history_cap);
    std::vector<float4> prev;
    const float4* hp[PLANES] = {};
    if (h_hist_prev) {
        prev.resize(PLANES * n);
        for (size_t i = 0; i < PLANES * n; i++) prev[i] = f4(h_hist_prev, i);
        for (int i = 0; i < PLANES; i++) hp[i] = prev.data() + i * n;
    }
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * (size_t)W + (size_t)x;
            const float* h = reinterpret_cast<const float*>(h_hits + p);
            const float* sr = reinterpret_cast<const float*>(h_surface + p);
            const float4 hit[3] = {f4(h, 0), f4(h, 1), f4(h, 2)};
            const int32_t k = tp_motion_index(hit[0], n_nodes);
            TpMotion T = host_motion(motion, k);
            f3 src[2];
            const bool ok = tp_deform_source(dh.D, k, T, f4(sr, 0), f4(sr, 1), mk3(hit[1].x, hit[1].y, hit[1].z), mk3(hit[2].x, hit[2].y, hit[2].z), src[0], src[1]);
            float4 out, o[PLANES];
            tp_pixel<true, MOMENTS, false, false, TpPinhole, true>(A, k >= 0, T, hp, x, y, f4(h_rgbz, p), hit, f4(h_albedo, p), out, o, true, nullptr, TpPinhole(),
                                                                   src, ok);
            st4(h_rgbz_out, p, out);
            for (int i = 0; i < PLANES; i++) st4(h_hist_out, i * n + p, o[i]);
        }
    return RTU_OK;
}

// the host loop of the sensor forms for one model: tp_pixel<false, MOMENTS> with that model's projection
template <int MODEL, bool MOMENTS>
static void accumulate_sensor_pixels(const TpParams& A, const RtuSensorDesc& prev, const float* h_rgbz, const RtuRayHit* h_hits, const float* h_albedo,
                                     const float4* const* hp, float* h_hist_out, float* h_rgbz_out) {
    constexpr int PLANES = MOMENTS ? 4 : 3;
    const size_t n = (size_t)A.width * (size_t)A.height;
    const TpSensorProj<MODEL> proj{prev};
    for (int y = 0; y < A.height; y++)
        for (int x = 0; x < A.width; x++) {
            const size_t p = (size_t)y * (size_t)A.width + (size_t)x;
            const float* h = reinterpret_cast<const float*>(h_hits + p);
            const float4 hit[3] = {f4(h, 0), f4(h, 1), f4(h, 2)};
            float4 out, o[PLANES];
            tp_pixel<false, MOMENTS, false, false, TpSensorProj<MODEL>>(A, false, tp_motion_identity(), hp, x, y, f4(h_rgbz, p), hit, f4(h_albedo, p), out, o,
                                                                        true, nullptr, proj);
            st4(h_rgbz_out, p, out);  // (the input pixel was read before: h_rgbz_out may be h_rgbz)
            for (int i = 0; i < PLANES; i++) st4(h_hist_out, i * n + p, o[i]);
        }
}

// the host forms for sensors: the histories have three planes, with MOMENTS four
template <bool MOMENTS>
static int accumulate_sensor_host(const RtuTemporalDesc* desc, const RtuSensorDesc* prev, const RtuSensorDesc* cur, const float* h_rgbz, const RtuRayHit* h_hits,
                                  const float* h_albedo, const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out) {
    constexpr int PLANES = MOMENTS ? 4 : 3;
    if (rtu_temporal_check_desc(desc) != RTU_OK || !cur || !h_rgbz || !h_hits || !h_albedo || !h_hist_out || !h_rgbz_out) return RTU_ERR_ARG;
    if (h_hist_prev && !prev) return RTU_ERR_ARG;
    if (!prev) prev = cur;
    if (rtu_sensor_check_desc(cur) != RTU_OK || rtu_sensor_check_desc(prev) != RTU_OK) return RTU_ERR_ARG;
    if (cur->width != desc->width || cur->height != desc->height) return RTU_ERR_ARG;
    const size_t n = (size_t)desc->width * (size_t)desc->height;
    if (h_hist_prev) {  // taps read anywhere in the previous history
        const uintptr_t a = (uintptr_t)h_hist_prev, b = (uintptr_t)h_hist_out, bytes = 16 * PLANES * n;
        if (a < b + bytes && b < a + bytes) return RTU_ERR_ARG;
    }
    const TpParams A = tp_sensor_setup(*desc, *prev, *cur, h_hist_prev != nullptr);
    std::vector<float4> planes;  // (the planes as float4: the caller's floats need not be 16-byte aligned)
    const float4* hp[PLANES] = {};
    if (A.lookup != TP_LOOKUP_NONE) {  // (else the previous history may be of another size, and is not read)
        planes.resize(PLANES * n);
        for (size_t i = 0; i < PLANES * n; i++) planes[i] = f4(h_hist_prev, i);
        for (int i = 0; i < PLANES; i++) hp[i] = planes.data() + i * n;
    }
    switch (prev->model) {
    case RTU_SENSOR_EQUIRECT: accumulate_sensor_pixels<RTU_SENSOR_EQUIRECT, MOMENTS>(A, *prev, h_rgbz, h_hits, h_albedo, hp, h_hist_out, h_rgbz_out); break;
    case RTU_SENSOR_FISHEYE: accumulate_sensor_pixels<RTU_SENSOR_FISHEYE, MOMENTS>(A, *prev, h_rgbz, h_hits, h_albedo, hp, h_hist_out, h_rgbz_out); break;
    default: accumulate_sensor_pixels<RTU_SENSOR_ORTHO, MOMENTS>(A, *prev, h_rgbz, h_hits, h_albedo, hp, h_hist_out, h_rgbz_out); break;
    }
    return RTU_OK;
}

extern "C" {

int rtu_temporal_accumulate_sensor(const RtuTemporalDesc* desc, const RtuSensorDesc* prev, const RtuSensorDesc* cur, const float* h_rgbz, const RtuRayHit* h_hits,
                                   const float* h_albedo, const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out) {
    return accumulate_sensor_host<false>(desc, prev, cur, h_rgbz, h_hits, h_albedo, h_hist_prev, h_hist_out, h_rgbz_out);
}

int rtu_temporal_accumulate_sensor_moments(const RtuTemporalDesc* desc, const RtuSensorDesc* prev, const RtuSensorDesc* cur, const float* h_rgbz,
                                           const RtuRayHit* h_hits, const float* h_albedo, const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out) {
    return accumulate_sensor_host<true>(desc, prev, cur, h_rgbz, h_hits, h_albedo, h_hist_prev, h_hist_out, h_rgbz_out);
}

int rtu_temporal_defaults(RtuTemporalDesc* out) {
    if (!out) return RTU_ERR_ARG;
    *out = RtuTemporalDesc{};
    out->max_history = 32;
    out->sigma_plane = 0.05f;
    out->normal_min = 0.9f;
    return RTU_OK;
}

int rtu_temporal_accumulate(const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam, const float* h_rgbz,
                            const RtuRayHit* h_hits, const float* h_albedo, const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out) {
    return accumulate_host<false, false>(desc, prev_cam, cur_cam, h_rgbz, h_hits, h_albedo, h_hist_prev, h_hist_out, h_rgbz_out, nullptr, 0, 0);
}

int rtu_temporal_accumulate_motion(const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam, const float* h_rgbz,
                                   const RtuRayHit* h_hits, const float* h_albedo, const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out,
                                   const RtuNodeMotion* motion, uint32_t n_nodes, int32_t history_cap) {
    return accumulate_host<true, false>(desc, prev_cam, cur_cam, h_rgbz, h_hits, h_albedo, h_hist_prev, h_hist_out, h_rgbz_out, motion, n_nodes, history_cap);
}

int rtu_temporal_accumulate_moments(const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam, const float* h_rgbz,
                                    const RtuRayHit* h_hits, const float* h_albedo, const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out,
                                    const RtuNodeMotion* motion, uint32_t n_nodes, int32_t history_cap) {
    return accumulate_host<true, true>(desc, prev_cam, cur_cam, h_rgbz, h_hits, h_albedo, h_hist_prev, h_hist_out, h_rgbz_out, motion, n_nodes, history_cap);
}

int rtu_temporal_accumulate_gradient(const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam, const float* h_rgbz,
                                     const RtuRayHit* h_hits, const float* h_albedo, const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out,
                                     const RtuNodeMotion* motion, uint32_t n_nodes, int32_t history_cap, const float* h_lambda) {
    return accumulate_host<true, true, true>(desc, prev_cam, cur_cam, h_rgbz, h_hits, h_albedo, h_hist_prev, h_hist_out, h_rgbz_out, motion, n_nodes,
                                             history_cap, h_lambda);
}

int rtu_temporal_accumulate_sparse(const RtuTemporalDesc* desc, const RtuSparseDesc* sparse_desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam,
                                   const float* h_rgbt, const uint32_t* owner, const RtuRayHit* h_hits, const float* h_albedo, const float* h_hist_prev,
                                   float* h_hist_out, float* h_rgbz_out, uint8_t* h_hole_out, const RtuNodeMotion* motion, uint32_t n_nodes,
                                   int32_t history_cap) {
    const SparseHost sp{sparse_desc, h_rgbt, owner, h_hole_out};
    return accumulate_host<true, true, false, true>(desc, prev_cam, cur_cam, nullptr, h_hits, h_albedo, h_hist_prev, h_hist_out, h_rgbz_out, motion, n_nodes,
                                                    history_cap, nullptr, &sp);
}

int rtu_temporal_accumulate_deform(const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam, const float* h_rgbz,
                                   const RtuRayHit* h_hits, const float* h_albedo, const RtuRaySurface* h_surface, const RtuSceneDesc* prev_scene,
                                   const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out, const RtuNodeMotion* motion, uint32_t n_nodes,
                                   int32_t history_cap) {
    return accumulate_deform_host<false>(desc, prev_cam, cur_cam, h_rgbz, h_hits, h_albedo, h_surface, prev_scene, h_hist_prev, h_hist_out, h_rgbz_out, motion,
                                         n_nodes, history_cap);
}

int rtu_temporal_accumulate_deform_moments(const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuFrameDesc* cur_cam, const float* h_rgbz,
                                           const RtuRayHit* h_hits, const float* h_albedo, const RtuRaySurface* h_surface, const RtuSceneDesc* prev_scene,
                                           const float* h_hist_prev, float* h_hist_out, float* h_rgbz_out, const RtuNodeMotion* motion, uint32_t n_nodes,
                                           int32_t history_cap) {
    return accumulate_deform_host<true>(desc, prev_cam, cur_cam, h_rgbz, h_hits, h_albedo, h_surface, prev_scene, h_hist_prev, h_hist_out, h_rgbz_out, motion,
                                        n_nodes, history_cap);
}

int rtu_motion_vectors_deform(const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuRayHit* h_hits, const RtuRaySurface* h_surface,
                              const RtuSceneDesc* prev_scene, const RtuNodeMotion* motion, uint32_t n_nodes, float* h_mv) {
    if (rtu_temporal_check_desc(desc) != RTU_OK || !prev_cam || !h_hits || !h_surface || !motion || !h_mv) return RTU_ERR_ARG;
    if (rtu_temporal_check_motion(motion, n_nodes, 0, true) != RTU_OK) return RTU_ERR_ARG;
    if (prev_cam->width != desc->width || prev_cam->height != desc->height) return RTU_ERR_ARG;
    DeformHost dh;
    if (!deform_host_setup(prev_scene, n_nodes, dh)) return RTU_ERR_ARG;
    const TpParams P = tp_setup(*desc, *prev_cam, *prev_cam, true);
    const size_t n = (size_t)desc->width * (size_t)desc->height;
    for (size_t p = 0; p < n; p++) {
        const float* h = reinterpret_cast<const float*>(h_hits + p);
        const float* sr = reinterpret_cast<const float*>(h_surface + p);
        const float4 hit[3] = {f4(h, 0), f4(h, 1), f4(h, 2)};
        const int32_t k = tp_motion_index(hit[0], n_nodes);
        TpMotion T = host_motion(motion, k);
        f3 src[2];
        const bool ok = tp_deform_source(dh.D, k, T, f4(sr, 0), f4(sr, 1), mk3(hit[1].x, hit[1].y, hit[1].z), mk3(hit[2].x, hit[2].y, hit[2].z), src[0], src[1]);
        st4(h_mv, p, tp_motion_vector_deform(P, k >= 0, T, src, ok));
    }
    return RTU_OK;
}

int rtu_motion_vectors(const RtuTemporalDesc* desc, const RtuFrameDesc* prev_cam, const RtuRayHit* h_hits, const RtuNodeMotion* motion, uint32_t n_nodes,
                       float* h_mv) {
    if (rtu_temporal_check_desc(desc) != RTU_OK || !prev_cam || !h_hits || !motion || !h_mv) return RTU_ERR_ARG;
    if (rtu_temporal_check_motion(motion, n_nodes, 0) != RTU_OK) return RTU_ERR_ARG;
    if (prev_cam->width != desc->width || prev_cam->height != desc->height) return RTU_ERR_ARG;
    const TpParams P = tp_setup(*desc, *prev_cam, *prev_cam, true);
    const size_t n = (size_t)desc->width * (size_t)desc->height;
    for (size_t p = 0; p < n; p++) {
        const float* h = reinterpret_cast<const float*>(h_hits + p);
        const float4 hit[3] = {make_float4(h[0], h[1], h[2], h[3]), make_float4(h[4], h[5], h[6], h[7]), make_float4(h[8], h[9], h[10], h[11])};
        const int32_t k = tp_motion_index(hit[0], n_nodes);
        const float4 v = tp_motion_vector(P, k >= 0, host_motion(motion, k), hit);
        h_mv[4 * p] = v.x; h_mv[4 * p + 1] = v.y; h_mv[4 * p + 2] = v.z; h_mv[4 * p + 3] = v.w;
    }
    return RTU_OK;
}

}  // extern "C"
