// rtu_sensor_adaptive.h — the launch interface of adaptive sensors (include/rtu_render.h, "Adaptive sensors"; rtu_sensor_adaptive.hip),
// called by rtu_capi_sensor.hip: the rays of the pixels that still sample, and the stopping rule applied to what comes back.
#ifndef RTU_SENSOR_ADAPTIVE_H_INCLUDED
#define RTU_SENSOR_ADAPTIVE_H_INCLUDED

#include "rtu_sensor.h"

#define RTU_SA_BLOCK 256u  // lanes per block of k_sa_step: the unit of the survivors' compaction

// One batch of `batch` samples [done, done + batch) of the live_n pixels of `list` (ascending pixel indices; nullptr: every pixel, the
// first batch), shaded into samples[b * live_n + i].
struct SaStep {
    const float4*   samples;
    const uint32_t* list;
    float4*         s;         // per pixel: the sums of r, g, b and of t over the hits
    float4*         q;         // per pixel: the sums of r^2, g^2, b^2, and the hit count (an integer in .w)
    float4*         out;       // the image: written when a pixel stops
    uint8_t*        counts;    // its sample counts, or nullptr
    uint32_t*       list_out;  // the survivors in ascending order, *n_out of them
    uint32_t*       n_out;
    uint32_t*       packed;    // scratch: rtu_sa_blocks(pixels) * RTU_SA_BLOCK words, the survivors of each block
    uint32_t*       blk;       // scratch: 2 * rtu_sa_blocks(pixels) words, the survivors per block and their exclusive scan
    const uint32_t* skip_if;   // two words each (FrameCounters::overflow, tail_declined; the side counters' flags): where one is set the host
    const uint32_t* skip_if_side;  // will shade the batch again, and the three kernels change nothing
    uint32_t        live_n, batch, done;
    uint32_t        max_samples, min_samples, increment;
    uint32_t        checkpoint;  // the first checkpoint n > done: min_samples + k * increment
    float           target;
};
inline uint32_t rtu_sa_blocks(size_t n) { return (uint32_t)((n + RTU_SA_BLOCK - 1u) / RTU_SA_BLOCK); }

// Every function is asynchronous on `stream` and returns a hipError_t as int.
// rays[(k * live_n + i) * 2 ..] and keys[k * live_n + i] of pixel list[i], sample off.sample[k] for k < n_samples <= RTU_SENSOR_LAUNCH_SAMPLES:
// the bits of rtu_sensor_rays. d validated; rays 16-byte aligned.
int rtu_launch_sa_rays(const RtuSensorDesc& d, const SensorOffsets& off, uint32_t n_samples, const uint32_t* list, uint32_t live_n, float4* rays,
                       uint32_t* keys, hipStream_t stream);
// k_sa_step, k_sa_scan, k_sa_gather: the rule of rtu_render.h in sample order, then the next list and its length.
int rtu_launch_sa_step(const SaStep& p, hipStream_t stream);

#endif
