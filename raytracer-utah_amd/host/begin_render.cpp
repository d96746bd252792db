// begin_render.cpp — the BeginRender()/StopRender() drop-in (main.cpp:29-72,
// viewport.cpp:36-37: "renderer must run in a separate thread").
//
// The reference detaches one coordinator thread that spawns hardware_concurrency() CPU workers, busy-waits, then
// writes Result.png and ZBuffer.png (main.cpp:29-64). Here the coordinator is ONE host thread that hands the frame to
// the C-ABI's multi-GPU entry (rtu_render.h: rtu_create_context_multi / rtu_multi_render_frame — one context per GPU,
// interleaved 8-row bands, the shards gathered over xGMI with RCCL or by concurrent copies; csrc/rtu_multi.hip), gets the
// bands back as they arrive, applies the reference's gamma / Color24 / z post-pass to each (image.cpp: the rendered-pixel
// counter of the RenderImage mirror advances band by band, scene.h:585-588) and writes the PNGs. No busy spin.
// StopRender() raises the cancel word the library polls (between the sample batches of recipes S / P, between capacity
// rounds, between the shards as they are handed over). It is written and read with relaxed atomics: rtu_stop_render runs on another
// thread than the job.
// Progressive display (rtu_begin_render_progressive): one progressive session per shard (rtu_render.h), advanced pass by pass; after
// every pass the image holds the pass's snapshot, so a viewport that polls it sees the frame refine, and a stop keeps the last pass.
#include "host_internal.h"
#include "rtu_render.h"

#include <algorithm>
#include <atomic>
#include <functional>
#include <string>
#include <thread>
#include <vector>

struct RtuRenderJob {
    std::thread       thread;
    volatile int      cancel = 0;      // polled by the library (RtuProgress::cancel); written with __atomic_store_n
    std::atomic<int>  result{1};       // 1 = running, 0 = ok, <0 = error
    std::atomic<int>  gather_kind{0};  // how the shards were collected: 1 one context, 2 asynchronous host copies, 3 RCCL
    std::string       error;
};

namespace {

void rows_to_image(void* user, const float* rows, int row0, int nrows) {
    rtu_image_from_rgbz(static_cast<RtuImage*>(user), rows, row0, nrows);  // gamma, Color24, z; bumps the rendered-pixel counter
}

void run_job(RtuRenderJob* job, const RtuSceneDesc* desc, RtuImage* img, std::vector<int> devices, int samples, int gather_bounces,
             std::string result_png, std::string zbuffer_png) {
    const int W = rtu_image_width(img), H = rtu_image_height(img);
    int rc = RTU_OK;
    RtuMultiContext* m = rtu_create_context_multi(devices.data(), (int)devices.size(), &rc);
    if (!m) {
        job->error = rtu_error_string(rc);
        job->result.store(rc != RTU_OK ? rc : RTU_ERR_HIP);
        return;
    }
    RtuFrameDesc frame;
    rc = rtu_multi_upload_scene(m, desc);
    if (rc == RTU_OK) rc = rtu_frame_setup(&desc->camera, W, H, &frame);
    if (rc == RTU_OK) {
        frame.samples = samples;
        frame.gather_bounces = gather_bounces;
        RtuProgress progress;
        progress.cancel = &job->cancel;
        progress.rows_done = rows_to_image;
        progress.user = img;
        rc = rtu_multi_render_frame(m, &frame, nullptr, &progress);
    }
    if (rc != RTU_OK) job->error = rtu_multi_last_error(m);
    job->gather_kind.store(rtu_multi_gather_kind(m));
    rtu_destroy_context_multi(m);
    if (rc == RTU_OK) {
        // main.cpp:59-61
        if (!result_png.empty() && rtu_image_save_png(img, result_png.c_str()) != 0) { rc = RTU_ERR_ARG; job->error = "cannot write " + result_png; }
        rtu_image_compute_zimg(img);
        if (rc == RTU_OK && !zbuffer_png.empty() && rtu_image_save_zpng(img, zbuffer_png.c_str()) != 0) { rc = RTU_ERR_ARG; job->error = "cannot write " + zbuffer_png; }
    }
    job->result.store(rc);
}

// Adaptive sampling (rtu_begin_render_adaptive): one context per listed device, shard r of n on the r-th, each on a host thread of its
// own (rtu_render_frame_adaptive is synchronous); then the rows and counts of every shard go into the image, and main.cpp:59-63.
void run_adaptive_job(RtuRenderJob* job, const RtuSceneDesc* desc, RtuImage* img, std::vector<int> devices, int samples, int gather_bounces,
                      RtuAdaptiveDesc ad, std::string result_png, std::string zbuffer_png, std::string samplecount_png) {
    const int W = rtu_image_width(img), H = rtu_image_height(img), n = (int)devices.size();
    RtuFrameDesc frame;
    int rc = rtu_frame_setup(&desc->camera, W, H, &frame);
    if (rc != RTU_OK) {
        job->error = rtu_error_string(rc);
        job->result.store(rc);
        return;
    }
    frame.samples = samples;
    frame.gather_bounces = gather_bounces;
    frame.shard_count = n;
    std::vector<RtuFrameDesc> frames(n, frame);
    std::vector<std::vector<float>> rgbz(n);
    std::vector<std::vector<uint8_t>> counts(n);
    std::vector<int> rcs(n, RTU_OK);
    std::vector<std::string> errors(n);
    std::vector<std::thread> workers;
    for (int r = 0; r < n; r++) {
        frames[r].shard_rank = r;
        const size_t pixels = (size_t)rtu_shard_rows(&frames[r]) * (size_t)W;
        rgbz[r].resize(pixels * 4);
        counts[r].resize(pixels);
        workers.emplace_back([&, r]() {
            int e = RTU_OK;
            RtuContext* ctx = rtu_create_context(devices[r], &e);
            if (!ctx) { rcs[r] = e != RTU_OK ? e : RTU_ERR_HIP; errors[r] = rtu_error_string(rcs[r]); return; }
            e = rtu_set_cancel_flag(ctx, &job->cancel);
            if (e == RTU_OK) e = rtu_upload_scene(ctx, desc);
            if (e == RTU_OK) e = rtu_render_frame_adaptive(ctx, &frames[r], &ad, rgbz[r].data(), counts[r].data(), nullptr);
            if (e != RTU_OK) errors[r] = rtu_last_error(ctx);
            rcs[r] = e;
            rtu_destroy_context(ctx);
        });
    }
    for (std::thread& t : workers) t.join();
    for (int r = 0; r < n && rc == RTU_OK; r++)
        if (rcs[r] != RTU_OK) { rc = rcs[r]; job->error = errors[r]; }
    if (rc == RTU_OK) {
        for (int r = 0; r < n; r++)
            for (int lr = 0; lr < rtu_shard_rows(&frames[r]); lr++) {
                const int row = rtu_shard_global_row(&frames[r], lr);
                rtu_image_from_rgbz(img, rgbz[r].data() + (size_t)lr * W * 4, row, 1);
                rtu_image_fill_sample_count(img, counts[r].data() + (size_t)lr * W, row, 1);
            }
        job->gather_kind.store(n == 1 ? 1 : 2);
        // main.cpp:59-63 (the last two lines are commented out in the reference)
        if (!result_png.empty() && rtu_image_save_png(img, result_png.c_str()) != 0) { rc = RTU_ERR_ARG; job->error = "cannot write " + result_png; }
        rtu_image_compute_zimg(img);
        if (rc == RTU_OK && !zbuffer_png.empty() && rtu_image_save_zpng(img, zbuffer_png.c_str()) != 0) { rc = RTU_ERR_ARG; job->error = "cannot write " + zbuffer_png; }
        rtu_image_compute_sample_count_img(img);
        if (rc == RTU_OK && !samplecount_png.empty() && rtu_image_save_sample_count_png(img, samplecount_png.c_str()) != 0) {
            rc = RTU_ERR_ARG;
            job->error = "cannot write " + samplecount_png;
        }
    }
    job->result.store(rc);
}

const unsigned kPostThreads = 8;  // host threads of a progressive pass's post-pass (not the machine's core count: it may be shared)

// run fn(0) .. fn(n - 1) on n host threads and wait for them
void for_shards(int n, const std::function<void(int)>& fn) {
    std::vector<std::thread> th;
    for (int r = 0; r < n; r++) th.emplace_back(fn, r);
    for (std::thread& t : th) t.join();
}

// Progressive display: one context and one session per listed device, shard r of n on the r-th. The passes advance in lockstep; after
// each, the shards' snapshots go into the image (Color24, z, and counts when adaptive) and on_pass is called; the next pass starts when
// on_pass returns, so the image does not change while on_pass runs. A stop ends the current pass after its current batch: the image
// keeps the last complete pass, whose PNGs are written, and the job returns RTU_ERR_CANCELLED.
void run_progressive_job(RtuRenderJob* job, const RtuSceneDesc* desc, RtuImage* img, std::vector<int> devices, int samples, int gather_bounces,
                         bool adaptive, RtuAdaptiveDesc ad, std::vector<int> passes, RtuPassDone on_pass, void* user, std::string result_png,
                         std::string zbuffer_png, std::string samplecount_png) {
    const int W = rtu_image_width(img), H = rtu_image_height(img), n = (int)devices.size();
    RtuFrameDesc frame;
    int rc = rtu_frame_setup(&desc->camera, W, H, &frame);
    if (rc != RTU_OK) {
        job->error = rtu_error_string(rc);
        job->result.store(rc);
        return;
    }
    frame.samples = samples;
    frame.gather_bounces = gather_bounces;
    frame.shard_count = n;
    std::vector<RtuFrameDesc> frames(n, frame);
    std::vector<RtuContext*> ctx(n, nullptr);
    std::vector<RtuProgressive*> sess(n, nullptr);
    std::vector<std::vector<float>> rgbz(n);
    std::vector<std::vector<uint8_t>> counts(n);
    std::vector<int> rcs(n, RTU_OK);
    std::vector<std::string> errors(n);
    for (int r = 0; r < n; r++) {
        frames[r].shard_rank = r;
        const size_t pixels = (size_t)rtu_shard_rows(&frames[r]) * (size_t)W;
        rgbz[r].resize(pixels * 4);
        counts[r].resize(pixels);
    }
    auto settle = [&]() {  // the first error of the shards, a cancel only if nothing else went wrong
        int out = RTU_OK;
        for (int r = 0; r < n; r++)
            if (rcs[r] != RTU_OK && (out == RTU_OK || out == RTU_ERR_CANCELLED)) { out = rcs[r]; job->error = errors[r]; }
        return out;
    };
    for_shards(n, [&](int r) {
        int e = RTU_OK;
        ctx[r] = rtu_create_context(devices[r], &e);
        if (!ctx[r]) { rcs[r] = e != RTU_OK ? e : RTU_ERR_HIP; errors[r] = rtu_error_string(rcs[r]); return; }
        e = rtu_set_cancel_flag(ctx[r], &job->cancel);
        if (e == RTU_OK) e = rtu_upload_scene(ctx[r], desc);
        if (e == RTU_OK) sess[r] = rtu_progressive_begin(ctx[r], &frames[r], adaptive ? &ad : nullptr, &e);
        if (e != RTU_OK) { rcs[r] = e; errors[r] = rtu_last_error(ctx[r]); }
    });
    rc = settle();
    int shown = 0, done = 0;  // passes in the image, samples per pixel they hold
    for (size_t k = 0; k < passes.size() && rc == RTU_OK; k++) {
        for_shards(n, [&](int r) {
            int e = rtu_progressive_advance(sess[r], passes[k], rtu_context_stream(ctx[r]));
            if (e == RTU_OK) e = rtu_progressive_snapshot(sess[r], rgbz[r].data(), adaptive ? counts[r].data() : nullptr);
            if (e != RTU_OK) { rcs[r] = e; errors[r] = rtu_last_error(ctx[r]); }
        });
        if ((rc = settle()) != RTU_OK) break;
        // the gamma / Color24 post-pass is a binary64 pow per channel, about 0.15 s per 1920 x 1080 image on one core: the rows are
        // dealt round-robin to kPostThreads host threads (each row is written by one of them)
        const unsigned hw = std::thread::hardware_concurrency();
        const int nt = (int)std::min<unsigned>(kPostThreads, hw ? hw : 1u);
        for_shards(nt, [&](int t) {
            int k = 0;
            for (int r = 0; r < n; r++)
                for (int lr = 0; lr < rtu_shard_rows(&frames[r]); lr++, k++) {
                    if (k % nt != t) continue;
                    const int row = rtu_shard_global_row(&frames[r], lr);
                    rtu::image_rows(img, rgbz[r].data() + (size_t)lr * W * 4, row, 1, shown == 0);  // the pixel counter reaches W * H once
                    if (adaptive) rtu_image_fill_sample_count(img, counts[r].data() + (size_t)lr * W, row, 1);
                }
        });
        shown++;
        done += passes[k];
        if (on_pass) on_pass(user, done, shown);
    }
    for (int r = 0; r < n; r++) {
        rtu_progressive_free(sess[r]);
        rtu_destroy_context(ctx[r]);
    }
    job->gather_kind.store(n == 1 ? 1 : 2);
    if ((rc == RTU_OK || rc == RTU_ERR_CANCELLED) && shown > 0) {
        // main.cpp:59-63 on the last complete pass
        int wr = RTU_OK;
        if (!result_png.empty() && rtu_image_save_png(img, result_png.c_str()) != 0) { wr = RTU_ERR_ARG; job->error = "cannot write " + result_png; }
        rtu_image_compute_zimg(img);
        if (wr == RTU_OK && !zbuffer_png.empty() && rtu_image_save_zpng(img, zbuffer_png.c_str()) != 0) { wr = RTU_ERR_ARG; job->error = "cannot write " + zbuffer_png; }
        if (adaptive) {
            rtu_image_compute_sample_count_img(img);
            if (wr == RTU_OK && !samplecount_png.empty() && rtu_image_save_sample_count_png(img, samplecount_png.c_str()) != 0) {
                wr = RTU_ERR_ARG;
                job->error = "cannot write " + samplecount_png;
            }
        }
        if (rc == RTU_OK) rc = wr;
    }
    job->result.store(rc);
}

}  // namespace

extern "C" {

RtuRenderJob* rtu_begin_render_adaptive(const RtuScene* scene, RtuImage* img, const int* device_ids, int n_devices, int samples,
                                        int gather_bounces, const RtuAdaptiveDesc* adaptive, const char* result_png,
                                        const char* zbuffer_png, const char* samplecount_png) {
    if (!scene || !img || !device_ids || n_devices < 1 || samples < 1 || samples > 255 || (gather_bounces != 0 && gather_bounces != 4)) {
        rtu::set_error("rtu_begin_render_adaptive: bad arguments");
        return nullptr;
    }
    RtuAdaptiveDesc ad;
    if (adaptive) ad = *adaptive;
    else rtu_adaptive_defaults(&ad);
    RtuRenderJob* job = new RtuRenderJob;
    std::vector<int> devs(device_ids, device_ids + n_devices);
    job->thread = std::thread(run_adaptive_job, job, rtu_scene_desc(scene), img, devs, samples, gather_bounces, ad,
                              std::string(result_png ? result_png : ""), std::string(zbuffer_png ? zbuffer_png : ""),
                              std::string(samplecount_png ? samplecount_png : ""));
    return job;  // returns immediately, as BeginRender() must
}

RtuRenderJob* rtu_begin_render_progressive(const RtuScene* scene, RtuImage* img, const int* device_ids, int n_devices, int samples,
                                           int gather_bounces, const RtuAdaptiveDesc* adaptive, const int* pass_samples, int n_passes,
                                           RtuPassDone on_pass, void* user, const char* result_png, const char* zbuffer_png,
                                           const char* samplecount_png) {
    if (!scene || !img || !device_ids || n_devices < 1 || samples < 1 || (gather_bounces != 0 && gather_bounces != 4) ||
        (adaptive && samples > 255)) {
        rtu::set_error("rtu_begin_render_progressive: bad arguments");
        return nullptr;
    }
    std::vector<int> passes;
    if (!pass_samples) {  // 1, 1, 2, 4, 8, ...: every pass doubles the samples shown, the last one up to `samples`
        for (int done = 0; done < samples;) {
            const int k = std::min(std::max(done, 1), samples - done);
            passes.push_back(k);
            done += k;
        }
    } else {
        if (n_passes < 1) {
            rtu::set_error("rtu_begin_render_progressive: a schedule has at least one pass");
            return nullptr;
        }
        long long total = 0;
        for (int k = 0; k < n_passes; k++) {
            if (pass_samples[k] < 1) {
                rtu::set_error("rtu_begin_render_progressive: pass " + std::to_string(k) + " has " + std::to_string(pass_samples[k]) +
                               " samples; every pass has at least one");
                return nullptr;
            }
            total += pass_samples[k];
        }
        if (total != samples) {
            rtu::set_error("rtu_begin_render_progressive: the passes add up to " + std::to_string(total) + " samples, not " + std::to_string(samples));
            return nullptr;
        }
        passes.assign(pass_samples, pass_samples + n_passes);
    }
    RtuAdaptiveDesc ad{};
    if (adaptive) ad = *adaptive;
    RtuRenderJob* job = new RtuRenderJob;
    std::vector<int> devs(device_ids, device_ids + n_devices);
    job->thread = std::thread(run_progressive_job, job, rtu_scene_desc(scene), img, devs, samples, gather_bounces, adaptive != nullptr, ad, passes,
                              on_pass, user, std::string(result_png ? result_png : ""), std::string(zbuffer_png ? zbuffer_png : ""),
                              std::string(samplecount_png ? samplecount_png : ""));
    return job;  // returns immediately, as BeginRender() must
}

static RtuRenderJob* begin(const RtuScene* scene, RtuImage* img, const int* device_ids, int n_devices, int samples, int gather_bounces,
                           const char* result_png, const char* zbuffer_png) {
    if (!scene || !img || !device_ids || n_devices < 1 || samples < 0) {
        rtu::set_error("rtu_begin_render: bad arguments");
        return nullptr;
    }
    RtuRenderJob* job = new RtuRenderJob;
    std::vector<int> devs(device_ids, device_ids + n_devices);
    job->thread = std::thread(run_job, job, rtu_scene_desc(scene), img, devs, samples, gather_bounces, std::string(result_png ? result_png : ""),
                              std::string(zbuffer_png ? zbuffer_png : ""));
    return job;  // returns immediately, as BeginRender() must
}

RtuRenderJob* rtu_begin_render_sampled(const RtuScene* scene, RtuImage* img, const int* device_ids, int n_devices, int samples,
                                       const char* result_png, const char* zbuffer_png) {
    return begin(scene, img, device_ids, n_devices, samples, 0, result_png, zbuffer_png);
}

RtuRenderJob* rtu_begin_render_paths(const RtuScene* scene, RtuImage* img, const int* device_ids, int n_devices, int samples,
                                     const char* result_png, const char* zbuffer_png) {
    return begin(scene, img, device_ids, n_devices, samples, 4, result_png, zbuffer_png);
}

RtuRenderJob* rtu_begin_render(const RtuScene* scene, RtuImage* img, const int* device_ids, int n_devices,
                               const char* result_png, const char* zbuffer_png) {
    return rtu_begin_render_sampled(scene, img, device_ids, n_devices, 0, result_png, zbuffer_png);
}

void rtu_stop_render(RtuRenderJob* job) {
    if (job) __atomic_store_n(&job->cancel, 1, __ATOMIC_RELAXED);
}

int rtu_render_wait(RtuRenderJob* job) {
    if (!job) return RTU_ERR_ARG;
    if (job->thread.joinable()) job->thread.join();
    if (job->result.load() != RTU_OK) rtu::set_error(job->error);
    return job->result.load();
}

int rtu_render_gather_kind(RtuRenderJob* job) {
    if (!job) return 0;
    if (job->thread.joinable()) job->thread.join();
    return job->gather_kind.load();
}

void rtu_render_job_free(RtuRenderJob* job) {
    if (!job) return;
    if (job->thread.joinable()) job->thread.join();
    delete job;
}

}  // extern "C"
