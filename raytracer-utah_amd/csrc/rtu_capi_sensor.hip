// rtu_capi_sensor.hip — the sensor part of the host side of the C-ABI in include/rtu_render.h, split off rtu_capi.hip: the rules of
// RtuSensorDesc, the host and device forms of a sensor's rays, its image (rtu_render_sensor*), the adaptive sample loop
// (rtu_render_sensor_adaptive*) and the host form of its projection. What it uses of rtu_capi.hip is declared in rtu_capi.h, which
// also declares what it offers rtu_capi_temporal.hip: check_sensor and sensor_generate. Compiled like rtu_capi.hip with
// -ffp-contract=off: the host forms round as the kernels do.
#include "rtu_capi.h"
#include "rtu_sensor.h"
#include "rtu_sensor_adaptive.h"

#include <cmath>
#include <cstring>

// ---- sensors (rtu_sensor.h, rtu_sensor.hip): the rays of a panoramic, fisheye or orthographic sensor, and its image --------------

namespace {

const size_t kSensorPixels = (size_t)1 << 25;  // pixels of a sensor, and rays of one batch of its samples, at most

bool fin3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

}  // namespace

// the rules of RtuSensorDesc (rtu_render.h); ctx may be NULL (rtu_sensor_rays)
int check_sensor(RtuContext* ctx, const RtuSensorDesc* d) {
    if (!d) return fail(ctx, RTU_ERR_ARG, "sensor descriptor is NULL");
    if (d->model != RTU_SENSOR_EQUIRECT && d->model != RTU_SENSOR_FISHEYE && d->model != RTU_SENSOR_ORTHO)
        return fail(ctx, RTU_ERR_ARG, "unknown sensor model %d", d->model);
    if (d->width < 1 || d->height < 1) return fail(ctx, RTU_ERR_ARG, "bad sensor resolution");
    if ((size_t)d->width * (size_t)d->height > kSensorPixels) return fail(ctx, RTU_ERR_ARG, "a sensor has 2^25 pixels at most");
    if (!fin3(d->pos) || !fin3(d->right) || !fin3(d->up) || !fin3(d->forward) || !std::isfinite(d->fov_deg) || !std::isfinite(d->extent[0]) ||
        !std::isfinite(d->extent[1]))
        return fail(ctx, RTU_ERR_ARG, "a sensor field is not finite");
    const f3 fr[3] = {ld3(d->right), ld3(d->up), ld3(d->forward)};
    for (int a = 0; a < 3; a++) {
        if (fabsf(dot3(fr[a], fr[a]) - 1.0f) > 2e-3f) return fail(ctx, RTU_ERR_ARG, "right / up / forward must be of unit length");
        for (int b = a + 1; b < 3; b++)
            if (fabsf(dot3(fr[a], fr[b])) > 2e-3f) return fail(ctx, RTU_ERR_ARG, "right / up / forward must be orthogonal");
    }
    if (d->model == RTU_SENSOR_FISHEYE && !(d->fov_deg > 0.0f && d->fov_deg <= 360.0f)) return fail(ctx, RTU_ERR_ARG, "fov_deg must be in (0, 360]");
    if (d->model == RTU_SENSOR_ORTHO && !(d->extent[0] > 0.0f && d->extent[1] > 0.0f)) return fail(ctx, RTU_ERR_ARG, "extent must be > 0");
    if (d->samples < 0 || d->samples > 65536) return fail(ctx, RTU_ERR_ARG, "samples out of range");
    if (d->gather_bounces != 0 && (d->gather_bounces != RTU_GI_BOUNCES || d->samples < 1))
        return fail(ctx, RTU_ERR_ARG, "gather_bounces is 0 or %d (recipe P, with samples >= 1)", RTU_GI_BOUNCES);
    if (d->max_bounce < 0 || d->max_bounce > RTU_MAX_BOUNCE) return fail(ctx, RTU_ERR_ARG, "max_bounce out of range");
    if (d->flags & ~RTU_QUERY_REFERENCE_WALK) return fail(ctx, RTU_ERR_ARG, "unknown sensor flag bits 0x%x", d->flags & ~RTU_QUERY_REFERENCE_WALK);
    for (uint32_t r : d->reserved)
        if (r) return fail(ctx, RTU_ERR_ARG, "RtuSensorDesc.reserved must be 0");
    return RTU_OK;
}

namespace {

// the pixel offsets of sample k: launch()'s and rtu_camera_sample_rays' expressions; recipe W (samples == 0): the pixel centre
void sensor_offset(const RtuSensorDesc* d, int k, float& ox, float& oy) {
    if (d->samples == 0) { ox = oy = 0.5f; return; }
    const float pixelIncrement = (float)(1.0 / d->samples);
    const float currentOffset = (float)k * pixelIncrement;
    ox = currentOffset + halton(k, 4);
    oy = currentOffset + halton(k, 5);
}

void sensor_rows(const RtuSensorDesc* d, int sample, int row0, int nrows, RtuRay* rays_out, uint32_t* keys_out) {
    float ox, oy;
    sensor_offset(d, sample, ox, oy);
    for (int y = row0; y < row0 + nrows; y++)
        for (int x = 0; x < d->width; x++) {
            f3 org, dir;
            switch (d->model) {
            case RTU_SENSOR_EQUIRECT: sensor_ray<RTU_SENSOR_EQUIRECT>(*d, x, y, ox, oy, HostSinCos(), org, dir); break;
            case RTU_SENSOR_FISHEYE: sensor_ray<RTU_SENSOR_FISHEYE>(*d, x, y, ox, oy, HostSinCos(), org, dir); break;
            default: sensor_ray<RTU_SENSOR_ORTHO>(*d, x, y, ox, oy, HostSinCos(), org, dir); break;
            }
            const size_t i = (size_t)(y - row0) * (size_t)d->width + (size_t)x;
            RtuRay& r = rays_out[i];
            r.org[0] = org.x; r.org[1] = org.y; r.org[2] = org.z;
            r.tmax = RTU_BIGFLOAT;
            r.dir[0] = dir.x; r.dir[1] = dir.y; r.dir[2] = dir.z;
            r.reserved = 0;
            keys_out[i] = rtu_sample_key((uint32_t)x + (uint32_t)d->width * (uint32_t)y, (uint32_t)sample);
        }
}

}  // namespace

// queue the generator for samples [k0, k0 + n) of the sensor into d_rays / d_keys (sample-major), RTU_SENSOR_LAUNCH_SAMPLES per launch
int sensor_generate(RtuContext* ctx, const RtuSensorDesc* d, int k0, int n, float4* d_rays, uint32_t* d_keys, hipStream_t stream) {
    const size_t pixels = (size_t)d->width * (size_t)d->height;
    for (int done = 0; done < n; done += RTU_SENSOR_LAUNCH_SAMPLES) {
        const int m = n - done < RTU_SENSOR_LAUNCH_SAMPLES ? n - done : RTU_SENSOR_LAUNCH_SAMPLES;
        SensorOffsets off;
        memset(&off, 0, sizeof off);
        for (int j = 0; j < m; j++) {
            sensor_offset(d, k0 + done + j, off.ox[j], off.oy[j]);
            off.sample[j] = (uint32_t)(k0 + done + j);
        }
        const hipError_t e = (hipError_t)rtu_launch_sensor_rays(*d, off, (uint32_t)m, d_rays + 2 * pixels * (size_t)done,
                                                                d_keys ? d_keys + pixels * (size_t)done : nullptr, stream);
        if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "sensor ray launch: %s", hipGetErrorString(e));
    }
    return RTU_OK;
}

static_assert(sizeof(RtuSensorDesc) == 128, "RtuSensorDesc is 128 bytes");

extern "C" {

int rtu_sensor_defaults(RtuSensorDesc* out) {
    if (!out) return RTU_ERR_ARG;
    memset(out, 0, sizeof *out);
    out->model = RTU_SENSOR_EQUIRECT;
    out->width = out->height = 1;
    out->max_bounce = RTU_MAX_BOUNCE;
    out->right[0] = 1.0f;
    out->up[1] = 1.0f;
    out->forward[2] = -1.0f;
    out->fov_deg = 180.0f;
    out->extent[0] = out->extent[1] = 1.0f;
    return RTU_OK;
}

// the specification of a sensor's rays: sensor_ray of rtu_sensor.h on the host (this file is compiled with -ffp-contract=off)
int rtu_sensor_rays(const RtuSensorDesc* d, int sample, int row0, int nrows, RtuRay* rays_out, uint32_t* keys_out) {
    if (check_sensor(nullptr, d) != RTU_OK) return RTU_ERR_ARG;
    if (row0 < 0 || nrows < 0 || row0 > d->height || nrows > d->height - row0) return RTU_ERR_ARG;
    if (sample < 0 || sample >= (d->samples > 0 ? d->samples : 1)) return RTU_ERR_ARG;
    if (nrows && (!rays_out || !keys_out)) return RTU_ERR_ARG;
    sensor_rows(d, sample, row0, nrows, rays_out, keys_out);
    return RTU_OK;
}

int rtu_sensor_rays_device(RtuContext* ctx, const RtuSensorDesc* d, int sample0, int nsamples, void* d_rays, void* d_keys, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    const int rc = check_sensor(ctx, d);
    if (rc != RTU_OK) return rc;
    const int total = d->samples > 0 ? d->samples : 1;
    if (sample0 < 0 || nsamples < 0 || sample0 > total || nsamples > total - sample0) return fail(ctx, RTU_ERR_ARG, "samples outside the sensor's");
    if (nsamples == 0) return RTU_OK;
    if ((size_t)nsamples * (size_t)d->width * (size_t)d->height > ((size_t)1 << 26)) return fail(ctx, RTU_ERR_ARG, "more than 2^26 rays in one call");
    if (!d_rays) return fail(ctx, RTU_ERR_ARG, "ray pointer is NULL");
    if (((uintptr_t)d_rays & 15u) || ((uintptr_t)d_keys & 3u)) return fail(ctx, RTU_ERR_ARG, "the ray buffer must be 16-byte, the key buffer 4-byte aligned");
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    return sensor_generate(ctx, d, sample0, nsamples, (float4*)d_rays, (uint32_t*)d_keys, (hipStream_t)hip_stream);
}

// The sample loop of a sensor: per batch the rays and keys (k_sensor_rays), the launch path of the matching ray-batch entry into
// sn_out, the capacity check of shade_host — a batch that overflowed is shaded again —, then k_sensor_accumulate; the last one resolves.
int rtu_render_sensor_device(RtuContext* ctx, const RtuSensorDesc* d, void* d_rgbz, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    int rc = check_sensor(ctx, d);
    if (rc != RTU_OK) return rc;
    if (!d_rgbz) return fail(ctx, RTU_ERR_ARG, "image pointer is NULL");
    if ((uintptr_t)d_rgbz & 15u) return fail(ctx, RTU_ERR_ARG, "the device image must be 16-byte aligned");
    const size_t pixels = (size_t)d->width * (size_t)d->height;
    const bool sampled = d->samples > 0, paths = d->gather_bounces != 0;
    const int n = sampled ? d->samples : 1;
    size_t fit = kSensorPixels / pixels;
    if (fit > RTU_MAX_BATCH) fit = RTU_MAX_BATCH;
    const int batch = (int)fit < n ? (int)fit : n;
    RtuShadeDesc sd;
    rtu_shade_defaults(&sd);
    memcpy(sd.eye, d->pos, sizeof sd.eye);
    sd.max_bounce = d->max_bounce;
    sd.flags = d->flags;
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    const hipStream_t stream = (hipStream_t)hip_stream;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->sn_rays.grow(2 * pixels * (size_t)batch));
    RTU_HIP(ctx, ctx->sn_keys.grow(pixels * (size_t)batch));
    RTU_HIP(ctx, ctx->sn_out.grow(pixels * (size_t)batch));
    RTU_HIP(ctx, ctx->sn_acc.grow(pixels));
    RTU_HIP(ctx, ctx->sn_hits.grow(pixels));
    RtuFrameDesc f;  // what launch() takes for a ray batch, by the checks of the _device entries (RTU_ERR_STOCHASTIC for recipe W)
    if ((rc = shade_args(ctx, ctx->sn_rays.get(), ctx->sn_out.get(), pixels * (size_t)batch, &sd, true, &f, sampled, ctx->sn_keys.get(), paths)) != RTU_OK) return rc;
    float4* const rays = ctx->sn_rays.get();
    float4* const out = ctx->sn_out.get();
    const uint32_t* const keys = sampled ? ctx->sn_keys.get() : nullptr;
    const bool timing = ctx->sn_timing;  // (diagnostic: also waits for every batch's accumulation)
    if (timing && !ctx->sn_ev[0])
        for (hipEvent_t& e : ctx->sn_ev) RTU_HIP(ctx, hipEventCreate(&e));
    if (timing) RTU_HIP(ctx, hipEventRecord(ctx->sn_ev[4], stream));
    for (int i = 0; i < n; i += batch) {
        if (cancel_raised(ctx)) return fail(ctx, RTU_ERR_CANCELLED, "cancelled after %d of %d samples", i, n);
        const int nb = n - i < batch ? n - i : batch;
        const uint32_t m = (uint32_t)(pixels * (size_t)nb);
        if (timing) RTU_HIP(ctx, hipEventRecord(ctx->sn_ev[0], stream));
        if ((rc = sensor_generate(ctx, d, i, nb, rays, ctx->sn_keys.get(), stream)) != RTU_OK) return rc;
        if (timing) RTU_HIP(ctx, hipEventRecord(ctx->sn_ev[1], stream));
        if (paths && (rc = paths_chain(ctx, f, out, stream, rays, keys, m)) != RTU_OK) return rc;
        if ((rc = shade_until_fits(ctx, f, out, stream, rays, keys, m, paths,
                                   "recipe P with counters: frame records ran out; render the sensor once without RTU_QUERY_REFERENCE_WALK first")) != RTU_OK)
            return rc;
        const bool last = i + nb >= n;
        if (timing) RTU_HIP(ctx, hipEventRecord(ctx->sn_ev[2], stream));
        const hipError_t e = (hipError_t)rtu_launch_sensor_accumulate(out, (uint32_t)nb, ctx->sn_acc.get(), ctx->sn_hits.get(), (uint32_t)pixels, i == 0,
                                                                      last ? (float4*)d_rgbz : nullptr, (uint32_t)n, stream);
        if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "sensor accumulate launch: %s", hipGetErrorString(e));
        if (timing) {
            RTU_HIP(ctx, hipEventRecord(ctx->sn_ev[3], stream));
            RTU_HIP(ctx, hipEventSynchronize(ctx->sn_ev[3]));
            for (int k = 0; k < 2; k++) {
                float ms = 0;
                RTU_HIP(ctx, hipEventElapsedTime(&ms, ctx->sn_ev[2 * k], ctx->sn_ev[2 * k + 1]));
                ctx->sn_ms[k] += ms;
            }
        }
    }
    if (timing) RTU_HIP(ctx, hipEventRecord(ctx->sn_ev[5], stream));
    RTU_HIP(ctx, hipStreamSynchronize(stream));
    if (timing) {
        float ms = 0;
        RTU_HIP(ctx, hipEventElapsedTime(&ms, ctx->sn_ev[4], ctx->sn_ev[5]));
        ctx->sn_ms[2] += ms;
    }
    return RTU_OK;
}

int rtu_debug_sensor_timing(RtuContext* ctx, int on, float* ms_out3) {
    if (!ctx) return RTU_ERR_ARG;
    if (ms_out3) memcpy(ms_out3, ctx->sn_ms, sizeof ctx->sn_ms);
    memset(ctx->sn_ms, 0, sizeof ctx->sn_ms);
    ctx->sn_timing = on != 0;
    return RTU_OK;
}

int rtu_render_sensor(RtuContext* ctx, const RtuSensorDesc* d, float* h_rgbz) {
    if (!ctx) return RTU_ERR_ARG;
    int rc = check_sensor(ctx, d);
    if (rc != RTU_OK) return rc;
    if (!h_rgbz) return fail(ctx, RTU_ERR_ARG, "image pointer is NULL");
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    const size_t pixels = (size_t)d->width * (size_t)d->height;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->sn_img.grow(pixels));
    if ((rc = rtu_render_sensor_device(ctx, d, ctx->sn_img.get(), ctx->stream)) != RTU_OK) return rc;
    RTU_HIP(ctx, hipMemcpy(h_rgbz, ctx->sn_img.get(), sizeof(float4) * pixels, hipMemcpyDeviceToHost));
    return RTU_OK;
}

}  // extern "C"

// ---- adaptive sensors (rtu_sensor_adaptive.h, rtu_sensor_adaptive.hip): the sample loop of a sensor over the pixels that still sample ----

namespace {

// the arguments both forms share: a recipe S / P sensor with 1 .. 255 samples and a valid RtuAdaptiveDesc
int check_sensor_adaptive(RtuContext* ctx, const RtuSensorDesc* d, const RtuAdaptiveDesc* ad) {
    const int rc = check_sensor(ctx, d);
    if (rc != RTU_OK) return rc;
    if (d->samples < 1 || d->samples > 255) return fail(ctx, RTU_ERR_ARG, "an adaptive sensor has 1 .. 255 samples per pixel at most (sensor.samples)");
    return check_adaptive_desc(ctx, ad, d->samples);
}

// what shade_until_fits queues behind a batch: the step kernels, and the copy of the next list's length to where the host reads it
struct SaBehind {
    RtuContext* ctx;
    SaStep      p;
    hipStream_t stream;
};
int sa_behind(void* arg) {
    SaBehind& b = *static_cast<SaBehind*>(arg);
    const hipError_t e = (hipError_t)rtu_launch_sa_step(b.p, b.stream);
    if (e != hipSuccess) return fail(b.ctx, RTU_ERR_HIP, "adaptive sensor step launch: %s", hipGetErrorString(e));
    RTU_HIP(b.ctx, hipMemcpyAsync(b.ctx->sa_n_host.get(), b.p.n_out, sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream));
    return RTU_OK;
}

}  // namespace

extern "C" {

// The sample loop of an adaptive sensor: per batch the rays and keys of the live pixels (the first batch: every pixel, k_sensor_rays;
// then k_sa_rays over the list), the launch path of the matching ray-batch entry into sn_out, and behind it — ahead of the batch's one
// synchronisation — k_sa_step with the next list, whose length the host reads in that synchronisation. A batch that overflowed is
// shaded again; the step kernels have then left it alone.
int rtu_render_sensor_adaptive_device(RtuContext* ctx, const RtuSensorDesc* d, const RtuAdaptiveDesc* ad, void* d_rgbz, void* d_counts, void* hip_stream) {
    if (!ctx) return RTU_ERR_ARG;
    int rc = check_sensor_adaptive(ctx, d, ad);
    if (rc != RTU_OK) return rc;
    if (!d_rgbz) return fail(ctx, RTU_ERR_ARG, "image pointer is NULL");
    if ((uintptr_t)d_rgbz & 15u) return fail(ctx, RTU_ERR_ARG, "the device image must be 16-byte aligned");
    const size_t pixels = (size_t)d->width * (size_t)d->height;
    const bool paths = d->gather_bounces != 0;
    const int S = d->samples;
    int most = ad->max_batch > 0 ? ad->max_batch : RTU_MAX_BATCH;  // samples of a batch, at most
    if (most > S) most = S;
    size_t cap = pixels * (size_t)most;  // rays of a batch, at most
    if (cap > kSensorPixels) cap = kSensorPixels;
    RtuShadeDesc sd;
    rtu_shade_defaults(&sd);
    memcpy(sd.eye, d->pos, sizeof sd.eye);
    sd.max_bounce = d->max_bounce;
    sd.flags = d->flags;
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    const hipStream_t stream = (hipStream_t)hip_stream;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->sn_rays.grow(2 * cap));
    RTU_HIP(ctx, ctx->sn_keys.grow(cap));
    RTU_HIP(ctx, ctx->sn_out.grow(cap));
    RTU_HIP(ctx, ctx->sa_s.grow(pixels));
    RTU_HIP(ctx, ctx->sa_q.grow(pixels));
    for (DevBuf<uint32_t>& l : ctx->sa_list) RTU_HIP(ctx, l.grow(pixels));
    const size_t blocks = rtu_sa_blocks(pixels);
    RTU_HIP(ctx, ctx->sa_packed.grow(blocks * RTU_SA_BLOCK));
    RTU_HIP(ctx, ctx->sa_blk.grow(2 * blocks));
    RTU_HIP(ctx, ctx->sa_n.grow(1));
    RTU_HIP(ctx, ctx->sa_n_host.grow(1));
    RtuFrameDesc f;  // what launch() takes for a ray batch, by the checks of the _device entries
    if ((rc = shade_args(ctx, ctx->sn_rays.get(), ctx->sn_out.get(), cap, &sd, true, &f, true, ctx->sn_keys.get(), paths)) != RTU_OK) return rc;
    float4* const rays = ctx->sn_rays.get();
    float4* const out = ctx->sn_out.get();
    uint32_t* const keys = ctx->sn_keys.get();
    ctx->sa_trace.clear();
    SaBehind behind;
    behind.ctx = ctx;
    behind.stream = stream;
    SaStep& p = behind.p;
    p.samples = out;
    p.s = ctx->sa_s.get();
    p.q = ctx->sa_q.get();
    p.out = (float4*)d_rgbz;
    p.counts = (uint8_t*)d_counts;
    p.n_out = ctx->sa_n.get();
    p.packed = ctx->sa_packed.get();
    p.blk = ctx->sa_blk.get();
    p.skip_if = &ctx->fcnt.get()->overflow;
    p.skip_if_side = &ctx->fcnt_side.get()->overflow;
    p.max_samples = (uint32_t)S;
    p.min_samples = (uint32_t)ad->min_samples;
    p.increment = (uint32_t)ad->increment;
    p.target = ad->target_variance;
    int cur = 0, done = 0;
    uint32_t live_n = (uint32_t)pixels;
    while (live_n > 0) {  // (done < S: the pixels that reach S stop there)
        if (cancel_raised(ctx)) return fail(ctx, RTU_ERR_CANCELLED, "cancelled after %d of %d samples", done, S);
        int nb = (int)(kSensorPixels / live_n) < most ? (int)(kSensorPixels / live_n) : most;
        if (nb > S - done) nb = S - done;
        const uint32_t m = live_n * (uint32_t)nb;
        if (done == 0) {
            if ((rc = sensor_generate(ctx, d, 0, nb, rays, keys, stream)) != RTU_OK) return rc;
        } else {
            SensorOffsets off;
            memset(&off, 0, sizeof off);
            for (int j = 0; j < nb; j++) {
                sensor_offset(d, done + j, off.ox[j], off.oy[j]);
                off.sample[j] = (uint32_t)(done + j);
            }
            const hipError_t e = (hipError_t)rtu_launch_sa_rays(*d, off, (uint32_t)nb, ctx->sa_list[cur].get(), live_n, rays, keys, stream);
            if (e != hipSuccess) return fail(ctx, RTU_ERR_HIP, "adaptive sensor ray launch: %s", hipGetErrorString(e));
        }
        p.list = done == 0 ? nullptr : ctx->sa_list[cur].get();
        p.list_out = ctx->sa_list[cur ^ 1].get();
        p.live_n = live_n;
        p.batch = (uint32_t)nb;
        p.done = (uint32_t)done;
        p.checkpoint = done < ad->min_samples ? (uint32_t)ad->min_samples
                                              : (uint32_t)(ad->min_samples + ((done - ad->min_samples) / ad->increment + 1) * ad->increment);
        if (paths && (rc = paths_chain(ctx, f, out, stream, rays, keys, m)) != RTU_OK) return rc;
        if ((rc = shade_until_fits(ctx, f, out, stream, rays, keys, m, paths,
                                   "recipe P with counters: frame records ran out; render the sensor once without RTU_QUERY_REFERENCE_WALK first",
                                   sa_behind, &behind)) != RTU_OK)
            return rc;
        ctx->sa_trace.push_back(live_n);
        ctx->sa_trace.push_back((uint32_t)nb);
        live_n = *ctx->sa_n_host.get();  // (read in the batch's synchronisation)
        cur ^= 1;
        done += nb;
    }
    return RTU_OK;
}

int rtu_render_sensor_adaptive(RtuContext* ctx, const RtuSensorDesc* d, const RtuAdaptiveDesc* ad, float* h_rgbz, uint8_t* h_counts) {
    if (!ctx) return RTU_ERR_ARG;
    int rc = check_sensor_adaptive(ctx, d, ad);
    if (rc != RTU_OK) return rc;
    if (!h_rgbz) return fail(ctx, RTU_ERR_ARG, "image pointer is NULL");
    if (!ctx->has_scene) return fail(ctx, RTU_ERR_NO_SCENE, "no scene uploaded");
    const size_t pixels = (size_t)d->width * (size_t)d->height;
    RTU_HIP(ctx, hipSetDevice(ctx->device));
    RTU_HIP(ctx, ctx->sa_img.grow(pixels));
    RTU_HIP(ctx, ctx->sa_counts.grow(pixels));
    if ((rc = rtu_render_sensor_adaptive_device(ctx, d, ad, ctx->sa_img.get(), ctx->sa_counts.get(), ctx->stream)) != RTU_OK) return rc;
    RTU_HIP(ctx, hipMemcpy(h_rgbz, ctx->sa_img.get(), sizeof(float4) * pixels, hipMemcpyDeviceToHost));
    if (h_counts) RTU_HIP(ctx, hipMemcpy(h_counts, ctx->sa_counts.get(), pixels, hipMemcpyDeviceToHost));
    return RTU_OK;
}

int rtu_debug_sensor_adaptive_trace(RtuContext* ctx, uint32_t* live_out, uint32_t* batch_out, int capacity) {
    if (!ctx || capacity < 0) return RTU_ERR_ARG;
    const int n = (int)(ctx->sa_trace.size() / 2);
    for (int b = 0; b < n && b < capacity; b++) {
        if (live_out) live_out[b] = ctx->sa_trace[2 * (size_t)b];
        if (batch_out) batch_out[b] = ctx->sa_trace[2 * (size_t)b + 1];
    }
    return n;
}

// ---- what temporal accumulation for sensors needs of a sensor (rtu_sensor.h sensor_project): its rules without a context, and the
// projection. (The accumulator on device memory and the sensor frames of a session are in rtu_capi_temporal.hip.) -------------------
int rtu_sensor_check_desc(const RtuSensorDesc* d) { return check_sensor(nullptr, d); }

// the specification of a sensor's projection: sensor_project of rtu_sensor.h on the host (this file is compiled with -ffp-contract=off)
int rtu_sensor_project(const RtuSensorDesc* d, const float* points_xyz, size_t n, float* fxfy_out, uint8_t* ok_out) {
    if (check_sensor(nullptr, d) != RTU_OK) return RTU_ERR_ARG;
    if (n && (!points_xyz || !fxfy_out || !ok_out)) return RTU_ERR_ARG;
    for (size_t i = 0; i < n; i++) {
        const f3 P = mk3(points_xyz[3 * i], points_xyz[3 * i + 1], points_xyz[3 * i + 2]);
        float fx = 0.0f, fy = 0.0f;
        bool ok;
        switch (d->model) {
        case RTU_SENSOR_EQUIRECT: ok = sensor_project<RTU_SENSOR_EQUIRECT>(*d, P, fx, fy); break;
        case RTU_SENSOR_FISHEYE: ok = sensor_project<RTU_SENSOR_FISHEYE>(*d, P, fx, fy); break;
        default: ok = sensor_project<RTU_SENSOR_ORTHO>(*d, P, fx, fy); break;
        }
        fxfy_out[2 * i] = ok ? fx : 0.0f;
        fxfy_out[2 * i + 1] = ok ? fy : 0.0f;
        ok_out[i] = ok ? 1 : 0;
    }
    return RTU_OK;
}

}  // extern "C"
