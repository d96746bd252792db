// render_kernel.hip — dispatch of a launch sequence to the feature set's translation unit
// (render_feat*.hip, all instantiating render_impl.h) plus the small kernels that are not part
// of a launch sequence: recipe S / P accumulation, the RenderImage packer, the self-tests.
#include "rtu_intersect.h"

namespace {
// Self-test of the exact-division identity used by the slab and barycentric tests
// (rtu_intersect.h, fdiv): pseudo-random bit patterns (all exponents, subnormals, zeros,
// infinities, NaNs) plus same-exponent pairs; counts quotients whose bits differ from `/`.
// ------------------------------------------------------------------------------------
__global__ void k_selftest_fdiv(unsigned long long n_pairs, unsigned long long seed, unsigned long long* mismatches) {
    unsigned long long bad = 0;
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < n_pairs;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        unsigned long long x = (i + seed) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
        unsigned int nb = (unsigned int)x, db = (unsigned int)(x >> 32);
        unsigned int mode = (unsigned int)(i & 7u);
        if (mode == 1) db = (db & 0x007FFFFFu) | (nb & 0xFF800000u);          // same exponent: quotient near 1
        if (mode == 2) nb = (nb & 0x807FFFFFu) | 0x3F800000u;                   // n in [1,2)
        if (mode == 3) { nb &= 0x80FFFFFFu; db = (db & 0x80FFFFFFu) | 0x7E000000u; }  // tiny / huge -> subnormal quotients
        if (mode == 4) db &= 0x807FFFFFu;                                       // subnormal / zero divisor
        float n = __uint_as_float(nb), d = __uint_as_float(db);
        float q1 = n / d;
        float q2 = fdiv(n, 1.0 / (double)d);
        bool same = __float_as_uint(q1) == __float_as_uint(q2) || (q1 != q1 && q2 != q2);
        if (!same) bad++;
    }
    if (bad) atomicAdd(mismatches, bad);
}

// Self-test of the re-ordered sphere / plane tests (rtu_intersect.h): the fast form against the
// literal reference order, bit for bit (return value, z, front, p, N), on rays built to stress
// the places where they could differ — grazing the sphere / the square's edge, far away (cancelling
// discriminant), axis-parallel, starting on the surface, with every incoming h.z regime.
__global__ void k_selftest_prims(unsigned long long n_rays, unsigned long long seed, unsigned long long* mismatches) {
    unsigned long long bad = 0;
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < n_rays;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        unsigned long long x = (i + seed) * 0x9E3779B97F4A7C15ull;
        auto rnd = [&]() {  // uniform in [0,1)
            x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
            return (float)(x >> 40) * (1.0f / 16777216.0f);
        };
        const unsigned mode = (unsigned)(i % 12u);
        const float scale = mode < 4 ? 3.0f : mode < 6 ? 40.0f : mode < 8 ? 3000.0f : 2.0f;
        Ray r;
        r.p = mk3((rnd() * 2 - 1) * scale, (rnd() * 2 - 1) * scale, (rnd() * 2 - 1) * scale);
        // aim at a point on / near the unit sphere or the unit square, then perturb
        f3 tgt = mk3(rnd() * 2 - 1, rnd() * 2 - 1, rnd() * 2 - 1);
        const bool plane = (i & 1u) != 0;
        if (plane) {
            tgt.z = 0;
            if (mode % 3u == 0) tgt.x = (rnd() < 0.5f ? -1.0f : 1.0f) * (1.0f + (rnd() * 2 - 1) * 1e-5f);  // the square's edge
            if (mode % 3u == 1) tgt.y = (rnd() < 0.5f ? -1.0f : 1.0f) * (1.0f + (rnd() * 2 - 1) * 1e-6f);
        } else {
            tgt = norm3(tgt);
            if (mode % 3u == 0) {  // a ray tangent to the sphere at tgt (+- a hair)
                f3 tang = norm3(cross3(tgt, mk3(rnd() + 0.1f, rnd() - 0.5f, rnd() - 0.5f)));
                r.p = tgt * (1.0f + (rnd() * 2 - 1) * 1e-5f) - tang * (rnd() * scale);
            }
            if (mode == 9) r.p = tgt;                       // origin on the surface
            if (mode == 10) r.p = tgt * (rnd() * 0.999f);   // origin inside
        }
        r.dir = tgt - r.p;
        if (mode == 11) { r.dir.x = 0; if (rnd() < 0.5f) r.dir.y = 0; }  // axis-parallel
        if (rnd() < 0.5f) r.dir = norm3(r.dir);
        if (rnd() < 0.1f) r.dir = r.dir * (rnd() * 50.0f);
        const float zsel = rnd();
        Hit h0;
        fresh_hit(h0, zsel < 0.4f ? RTU_BIGFLOAT : zsel < 0.7f ? rnd() * 2.0f * scale : rnd() * 0.01f);
        h0.front = rnd() < 0.5f;
        Hit a = h0, b = h0;
        bool ra, rb;
        if (plane) { ra = plane_hit_t<true>(r, a); rb = plane_hit_t<false>(r, b); }
        else { ra = sphere_hit_t<true>(r, a); rb = sphere_hit_t<false>(r, b); }
        auto same = [](float u, float v) { return __float_as_uint(u) == __float_as_uint(v) || (u != u && v != v); };
        bool ok = ra == rb && same(a.z, b.z) && a.front == b.front;
        if (ra && rb) ok = ok && same(a.p.x, b.p.x) && same(a.p.y, b.p.y) && same(a.p.z, b.p.z) && same(a.N.x, b.N.x) && same(a.N.y, b.N.y) && same(a.N.z, b.N.z);
        if (!ok) bad++;
    }
    if (bad) atomicAdd(mismatches, bad);
}


// ---- recipe P ----
// the pixel of a chain: Shade(h_0, AmbientLight) + Shade(h_0, lights) (:134-135), z of the primary hit
__global__ void __launch_bounds__(256) k_gi_final(KernelArgs a) {
    const uint32_t chain = blockIdx.x * 256u + threadIdx.x;
    if (chain >= a.gi_total) return;
    const uint32_t pk = __float_as_uint(a.gi_h[(size_t)a.gi_total + chain].w);
    if (!(pk & 1u)) return;  // missed (background) or a node without material (white): written by the chain's first launch
    const float4 ra = a.gi_res[chain], rd = a.gi_res[(size_t)a.gi_total + chain];
    a.out[chain] = make_float4(ra.x + rd.x, ra.y + rd.y, ra.z + rd.z, a.gi_h[chain].w);
}

}  // namespace

// ---- recipe S: the sums of RenderFunctions.cpp:109-110,148 in sample order, and :152 -----------
namespace {
// the mean of a pixel's sums over n samples of which `hits` hit: rgb / n, z / hits (BIGFLOAT without a hit), each a binary32
// division. k_resolve, k_resolve_counts and k_progressive_snapshot all call this, so a snapshot is their image by construction.
__device__ __forceinline__ float4 resolve_mean(const float4& s, uint32_t hits, float n) {
    return make_float4(s.x / n, s.y / n, s.z / n, hits ? s.w / (float)hits : RTU_BIGFLOAT);
}

__global__ void __launch_bounds__(256) k_accumulate(const float4* samples, uint32_t batch, float4* acc, uint32_t* hits, uint32_t pixels, int first) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= pixels) return;
    float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint32_t n = 0;
    if (!first) { s = acc[i]; n = hits[i]; }
    for (uint32_t b = 0; b < batch; b++) {  // the samples of the batch in their order
        const float4 v = samples[(size_t)b * pixels + i];
        s.x += v.x; s.y += v.y; s.z += v.z;                // pixelValuesSum += currentResult
        if (v.w != RTU_BIGFLOAT) { s.w += v.w; n++; }      // zSum += z; numOfHits++
    }
    acc[i] = s;
    hits[i] = n;
}
__global__ void __launch_bounds__(256) k_resolve(const float4* acc, const uint32_t* hits, float4* out, uint32_t pixels, uint32_t samples) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= pixels) return;
    const float4 s = acc[i];
    const uint32_t n = hits[i];
    out[i] = resolve_mean(s, n, (float)samples);
}

// rtu_progressive_snapshot: the image of a session's running sums, which it leaves as they are. counts == nullptr: every pixel has
// `n` samples (a fixed session); else its own count (adaptive). counts_out (may be nullptr) receives that count.
__global__ void __launch_bounds__(256) k_progressive_snapshot(const float4* acc, const uint32_t* hits, const uint8_t* counts, uint32_t n, float4* out,
                                                              uint8_t* counts_out, uint32_t pixels) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= pixels) return;
    const float4 s = acc[i];
    const uint32_t h = hits[i];
    const uint32_t c = counts ? (uint32_t)counts[i] : n;
    out[i] = resolve_mean(s, h, (float)c);
    if (counts_out) counts_out[i] = (uint8_t)c;
}
}  // namespace

// ---- adaptive sampling (rtu_render_frame_adaptive): per pixel s += x, q += x * x in sample order, stop at the first checkpoint ------
// n = min_samples + k * increment < max_samples with (q - s * m) / (n - 1) <= target for r, g and b (m = s / n); rtu_render.h
namespace {
__global__ void __launch_bounds__(64) k_adaptive_init(uint4* list, uint32_t tiles, uint32_t tiles_x, int width, int height, int shard_rank, int shard_count) {
    const uint32_t tile = blockIdx.x * 64u + threadIdx.x;
    if (tile >= tiles) return;
    const uint32_t band_local = tile / tiles_x, tx = tile - band_local * tiles_x;
    const int x0 = (int)(tx * 8u), y0 = (int)((band_local * (uint32_t)shard_count + (uint32_t)shard_rank) * RTU_BAND_ROWS);
    unsigned long long m = 0;  // the lanes of primary_stage1 that lie inside the image
    for (int l = 0; l < 64; l++)
        if (x0 + (l & 7) < width && y0 + (l >> 3) < height) m |= 1ull << l;
    list[tile] = make_uint4(tile, 0u, (uint32_t)m, (uint32_t)(m >> 32));
}

__device__ __forceinline__ bool adaptive_passes(const float4& s, const float4& q, uint32_t n, float target) {
    if (n == 1u) return target == __builtin_inff();  // var = +inf
    const float fn = (float)n, fn1 = (float)(n - 1u);
    // every operation rounded on its own (__f*_rn: no contraction), in the order of the statement in rtu_render.h
    const float vr = __fsub_rn(q.x, __fmul_rn(s.x, s.x / fn)) / fn1;
    const float vg = __fsub_rn(q.y, __fmul_rn(s.y, s.y / fn)) / fn1;
    const float vb = __fsub_rn(q.z, __fmul_rn(s.z, s.z / fn)) / fn1;
    return vr <= target && vg <= target && vb <= target;
}

// one wavefront per entry of the active-tile list, one lane per pixel of its 8x8 tile
__global__ void __launch_bounds__(256) k_adaptive_step(AdaptiveStep p) {
    const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (e >= p.n_in) return;
    if (p.skip_if[0] | p.skip_if[1] | p.skip_if_side[0] | p.skip_if_side[1]) return;  // incomplete batch: rendered again, then added
    const uint32_t lane = threadIdx.x & 63u;
    const uint4 ent = p.list_in[e];
    const bool on = (((unsigned long long)ent.w << 32 | ent.z) >> lane) & 1ull;
    const uint32_t band_local = ent.x / p.tiles_x, tx = ent.x - band_local * p.tiles_x;
    const uint32_t pix = (band_local * RTU_BAND_ROWS + (lane >> 3)) * (uint32_t)p.width + tx * 8u + (lane & 7u);
    bool more = false;
    if (on) {
        float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q = s;
        uint32_t h = 0, n = 0;
        if (!p.first) { s = p.acc[pix]; q = p.sq[pix]; h = p.hits[pix]; n = p.counts[pix]; }
        more = true;
        for (uint32_t b = 0; b < p.batch && more; b++) {  // the samples of the batch in their order, up to the pixel's stop
            const float4 v = p.samples[(size_t)b * p.pixels + pix];
            s.x = __fadd_rn(s.x, v.x); s.y = __fadd_rn(s.y, v.y); s.z = __fadd_rn(s.z, v.z);                   // k_accumulate's sum
            q.x = __fadd_rn(q.x, __fmul_rn(v.x, v.x)); q.y = __fadd_rn(q.y, __fmul_rn(v.y, v.y)); q.z = __fadd_rn(q.z, __fmul_rn(v.z, v.z));
            if (v.w != RTU_BIGFLOAT) { s.w += v.w; h++; }
            n++;
            if (n >= p.max_samples) more = false;
            else if (n >= p.min_samples && (n - p.min_samples) % p.increment == 0u && adaptive_passes(s, q, n, p.target)) more = false;
        }
        p.acc[pix] = s;
        p.sq[pix] = q;
        p.hits[pix] = h;
        p.counts[pix] = (uint8_t)n;
    }
    const unsigned long long m = __ballot(more);
    if (lane == 0u && m) {  // one append per wavefront
        const uint32_t k = atomicAdd(p.n_out, 1u);
        p.list_out[k] = make_uint4(ent.x, 0u, (uint32_t)m, (uint32_t)(m >> 32));
    }
}

__global__ void __launch_bounds__(256) k_resolve_counts(const float4* acc, const uint32_t* hits, const uint8_t* counts, float4* out, uint8_t* counts_out, uint32_t pixels) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= pixels) return;
    const float4 s = acc[i];
    const uint32_t h = hits[i];
    const uint8_t c = counts[i];
    out[i] = resolve_mean(s, h, (float)c);
    if (counts_out) counts_out[i] = c;
}
}  // namespace

int rtu_launch_adaptive_init(uint4* list, uint32_t tiles, uint32_t tiles_x, int width, int height, int shard_rank, int shard_count, hipStream_t stream) {
    if (tiles == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_adaptive_init, dim3((tiles + 63u) / 64u), dim3(64), 0, stream, list, tiles, tiles_x, width, height, shard_rank, shard_count);
    return (int)hipGetLastError();
}
int rtu_launch_adaptive_step(const AdaptiveStep& p, hipStream_t stream) {
    if (p.n_in == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_adaptive_step, dim3((p.n_in + 3u) / 4u), dim3(256), 0, stream, p);
    return (int)hipGetLastError();
}
int rtu_launch_resolve_counts(const float4* acc, const uint32_t* hits, const uint8_t* counts, float4* out, uint8_t* counts_out, uint32_t pixels, hipStream_t stream) {
    if (pixels == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_resolve_counts, dim3((pixels + 255u) / 256u), dim3(256), 0, stream, acc, hits, counts, out, counts_out, pixels);
    return (int)hipGetLastError();
}

// ---- RenderImage content on the device: Color24 pixels + float z (RenderFunctions.cpp:152-160, cyColor.h:226,245) ----
namespace {
__device__ __forceinline__ uint8_t float_to_byte(float r) {  // Color24(Color): Clamp(int(c * 255)), cvttss2si semantics
    const int i = cvtt_i32(r * 255);
    return (uint8_t)(i < 0 ? 0 : (i > 255 ? 255 : i));
}
__global__ void __launch_bounds__(256) k_pack_image(const float4* rgbz, unsigned long long pixels, float* z_out, uint8_t* rgb_out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i >= pixels) return;
    const float4 v = rgbz[i];
    z_out[i] = v.w;
    rgb_out[3 * i + 0] = float_to_byte((float)pow((double)v.x, 1 / 2.2));  // pow(c, 1/2.2) in binary64, as the reference
    rgb_out[3 * i + 1] = float_to_byte((float)pow((double)v.y, 1 / 2.2));
    rgb_out[3 * i + 2] = float_to_byte((float)pow((double)v.z, 1 / 2.2));
}
}  // namespace

// ---- the two OUTPUT images of a frame, 4 bytes per pixel: Color24 + the z-image byte of ComputeZBufferImage (scene.h:590-612) ----
// The z-image needs the frame-wide zmin / zmax over the pixels that hit (z != BIGFLOAT). k_minmax_z reduces them per frame of a
// batch into order-preserving integer keys (min as key, max as ~key, so that ONE element-wise MIN over the shards of all GPUs
// combines both); k_pack_output then quantises with the reference's float expression (correctly rounded division, truncation).
namespace {
__device__ __forceinline__ uint32_t z_key(float z) {  // monotone: a < b  <=>  z_key(a) < z_key(b), all finite floats
    const uint32_t b = __float_as_uint(z);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float z_unkey(uint32_t k) { return __uint_as_float((k >> 31) ? (k & 0x7FFFFFFFu) : ~k); }

__global__ void __launch_bounds__(256) k_minmax_z(const float4* rgbz, uint32_t pixels_per_frame, long long* minmax) {
    const uint32_t frame = blockIdx.y;
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;  // nothing hit yet: zmin = BIGFLOAT, zmax = 0 are applied when the keys are read
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < pixels_per_frame; i += gridDim.x * 256u) {
        const float z = rgbz[(size_t)frame * pixels_per_frame + i].w;
        if (z == RTU_BIGFLOAT || z != z) continue;  // a miss; a NaN never wins a comparison in the reference's loop either
        const uint32_t k = z_key(z);
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t a = (uint32_t)__shfl_xor((int)kmin, off), b = (uint32_t)__shfl_xor((int)kmax, off);
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
    }
    if ((threadIdx.x & 63u) == 0) {
        if (kmin != 0xFFFFFFFFu) atomicMin((unsigned long long*)&minmax[2 * frame], (unsigned long long)kmin);
        if (kmax != 0u) atomicMin((unsigned long long*)&minmax[2 * frame + 1], (unsigned long long)(~kmax));
    }
}

__global__ void __launch_bounds__(256) k_pack_output(const float4* rgbz, uint32_t pixels_per_frame, const long long* minmax, uchar4* out) {
    const uint32_t frame = blockIdx.y;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= pixels_per_frame) return;
    // scene.h:596-601: float zmin = BIGFLOAT, zmax = 0, then min / max over the pixels that hit
    const unsigned long long kmin = (unsigned long long)minmax[2 * frame], nkmax = (unsigned long long)minmax[2 * frame + 1];
    float zmin = kmin > 0xFFFFFFFFull ? RTU_BIGFLOAT : z_unkey((uint32_t)kmin);
    float zmax = nkmax > 0xFFFFFFFFull ? 0.0f : z_unkey(~(uint32_t)nkmax);
    if (!(RTU_BIGFLOAT > zmin)) zmin = RTU_BIGFLOAT;  // `if (zmin > z) zmin = z` starting from BIGFLOAT: never above it
    if (!(0.0f < zmax)) zmax = 0.0f;                  // `if (zmax < z) zmax = z` starting from 0: never below it
    const float4 v = rgbz[(size_t)frame * pixels_per_frame + i];
    uchar4 o;
    o.x = float_to_byte((float)pow((double)v.x, 1 / 2.2));
    o.y = float_to_byte((float)pow((double)v.y, 1 / 2.2));
    o.z = float_to_byte((float)pow((double)v.z, 1 / 2.2));
    o.w = v.w == RTU_BIGFLOAT ? (uint8_t)0 : float_to_byte((zmax - v.w) / (zmax - zmin));  // :603-609 (float_to_byte = int(f * 255), clamped)
    out[(size_t)frame * pixels_per_frame + i] = o;
}
}  // namespace

int rtu_launch_minmax_z(const float4* rgbz, uint32_t pixels_per_frame, uint32_t frames, long long* minmax, hipStream_t stream) {
    if (pixels_per_frame == 0 || frames == 0) return (int)hipSuccess;
    hipError_t e = hipMemsetAsync(minmax, 0x7F, sizeof(long long) * 2 * frames, stream);  // "nothing yet": any key is below 0x7F7F...
    if (e != hipSuccess) return (int)e;
    uint32_t bx = (pixels_per_frame + 255u) / 256u;
    if (bx > 1024u) bx = 1024u;
    hipLaunchKernelGGL(k_minmax_z, dim3(bx, frames), dim3(256), 0, stream, rgbz, pixels_per_frame, minmax);
    return (int)hipGetLastError();
}

int rtu_launch_pack_output(const float4* rgbz, uint32_t pixels_per_frame, uint32_t frames, const long long* minmax, unsigned char* out, hipStream_t stream) {
    if (pixels_per_frame == 0 || frames == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_pack_output, dim3((pixels_per_frame + 255u) / 256u, frames), dim3(256), 0, stream, rgbz, pixels_per_frame, minmax, (uchar4*)out);
    return (int)hipGetLastError();
}

int rtu_launch_pack_image(const float4* rgbz, unsigned long long pixels, float* z_out, unsigned char* rgb_out, hipStream_t stream) {
    if (pixels == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_pack_image, dim3((unsigned)((pixels + 255u) / 256u)), dim3(256), 0, stream, rgbz, pixels, z_out, (uint8_t*)rgb_out);
    return (int)hipGetLastError();
}

int rtu_launch_accumulate(const float4* samples, uint32_t batch, float4* acc, uint32_t* hits, uint32_t pixels, bool first, hipStream_t stream) {
    hipLaunchKernelGGL(k_accumulate, dim3((pixels + 255u) / 256u), dim3(256), 0, stream, samples, batch, acc, hits, pixels, first ? 1 : 0);
    return (int)hipGetLastError();
}
int rtu_launch_resolve(const float4* acc, const uint32_t* hits, float4* out, uint32_t pixels, uint32_t samples, hipStream_t stream) {
    hipLaunchKernelGGL(k_resolve, dim3((pixels + 255u) / 256u), dim3(256), 0, stream, acc, hits, out, pixels, samples);
    return (int)hipGetLastError();
}

int rtu_launch_progressive_snapshot(const float4* acc, const uint32_t* hits, const uint8_t* counts, uint32_t n, float4* out, uint8_t* counts_out,
                                    uint32_t pixels, hipStream_t stream) {
    if (pixels == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_progressive_snapshot, dim3((pixels + 255u) / 256u), dim3(256), 0, stream, acc, hits, counts, n, out, counts_out, pixels);
    return (int)hipGetLastError();
}

// DevNode::plane_n: one thread per node. The expressions are the pixels' own — from_node for the node and each ancestor in trace()'s
// order — in this translation unit's binary32 arithmetic, which is every render kernel's (the Makefile's flags): IEEE operations in a
// fixed order have one result. The plane's own normal (0, 0, +-1) arrives as kernel arguments (zero = 0, one = 1), as a value the
// compiler does not know: every operation is then executed by the instruction a pixel would execute it with, whatever a folded
// constant would make of a NaN's payload.
__global__ void __launch_bounds__(64) k_plane_normals(DevNode* nodes, uint32_t n_nodes, float zero, float one) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n_nodes || nodes[i].obj_type != RTU_OBJ_PLANE) return;
    for (int side = 0; side < 2; side++) {
        Hit h;
        fresh_hit(h, RTU_BIGFLOAT);
        h.N = mk3(zero, zero, side == 0 ? one : -one);  // plane_hit: front, back
        for (int j = (int)i; j >= 0; j = nodes[j].parent) from_node(nodes[j], h);
        nodes[i].plane_n[side][0] = h.N.x;
        nodes[i].plane_n[side][1] = h.N.y;
        nodes[i].plane_n[side][2] = h.N.z;
    }
}
int rtu_launch_plane_normals(DevNode* nodes, uint32_t n_nodes, hipStream_t stream) {
    if (n_nodes == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_plane_normals, dim3((n_nodes + 63u) / 64u), dim3(64), 0, stream, nodes, n_nodes, 0.0f, 1.0f);
    return (int)hipGetLastError();
}

int rtu_launch_selftest_fdiv(unsigned long long n_pairs, unsigned long long seed, unsigned long long* d_mismatches, hipStream_t stream) {
    hipLaunchKernelGGL(k_selftest_fdiv, dim3(4096), dim3(256), 0, stream, n_pairs, seed, d_mismatches);
    return (int)hipGetLastError();
}

int rtu_launch_selftest_prims(unsigned long long n_rays, unsigned long long seed, unsigned long long* d_mismatches, hipStream_t stream) {
    hipLaunchKernelGGL(k_selftest_prims, dim3(4096), dim3(256), 0, stream, n_rays, seed, d_mismatches);
    return (int)hipGetLastError();
}

// rtu_debug_texcoords: the texture arithmetic of the kernels, by the same __device__ functions, on n inputs of
// RTU_TEXOP_IN(op) floats each; RTU_TEXOP_OUT(op) floats out per input. `tex` has been checked by the caller.
__global__ void __launch_bounds__(256) k_debug_texcoords(DevScene s, int op, const DevTexture* tex, const RtuTexMap* map,
                                                         const float* in, float* out, unsigned long long n) {
    for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256ull) {
        if (op == RTU_TEXOP_ATAN2F) { out[i] = portable_atan2f(in[2 * i], in[2 * i + 1]); continue; }
        if (op == RTU_TEXOP_ASINF) { out[i] = portable_asinf(in[i]); continue; }
        const f3 a = mk3(in[3 * i], in[3 * i + 1], in[3 * i + 2]);
        f3 r;
        if (op == RTU_TEXOP_SPHERE_UV) r = sphere_uv(a);
        else if (op == RTU_TEXOP_ENV_UVW) r = env_uvw(a);
        else if (op == RTU_TEXOP_TILE_CLAMP) r = tile_clamp(a);
        else if (op == RTU_TEXOP_TEXTURE) r = texture_sample(*tex, a);
        else r = map_sample(s, *map, a);
        out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
    }
}
int rtu_launch_debug_texcoords(const DevScene& s, int op, const DevTexture* tex, const RtuTexMap* map, const float* in, float* out,
                               unsigned long long n, hipStream_t stream) {
    if (n == 0) return (int)hipSuccess;
    const unsigned long long blocks = (n + 255u) / 256u;
    hipLaunchKernelGGL(k_debug_texcoords, dim3((unsigned)(blocks < 8192u ? blocks : 8192u)), dim3(256), 0, stream, s, op, tex, map, in, out, n);
    return (int)hipGetLastError();
}


int rtu_launch_feat0(const KernelArgs& args, uint32_t n_tiles, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, int mode, const LaunchProbe* probe);
int rtu_launch_feat1(const KernelArgs& args, uint32_t n_tiles, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, int mode, const LaunchProbe* probe);
int rtu_launch_feat2(const KernelArgs& args, uint32_t n_tiles, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, int mode, const LaunchProbe* probe);
int rtu_launch_feat3(const KernelArgs& args, uint32_t n_tiles, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, int mode, const LaunchProbe* probe);
int rtu_launch_feat4(const KernelArgs& args, uint32_t n_tiles, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, int mode, const LaunchProbe* probe);
int rtu_launch_feat5(const KernelArgs& args, uint32_t n_tiles, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, int mode, const LaunchProbe* probe);
int rtu_launch_feat10(const KernelArgs& args, uint32_t n_tiles, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, int mode, const LaunchProbe* probe);
int rtu_launch_feat11(const KernelArgs& args, uint32_t n_tiles, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, int mode, const LaunchProbe* probe);
int rtu_launch_feat16(const KernelArgs& args, uint32_t n_tiles, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, int mode, const LaunchProbe* probe);
int rtu_launch_feat17(const KernelArgs& args, uint32_t n_tiles, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, int mode, const LaunchProbe* probe);
int rtu_launch_feat18(const KernelArgs& args, uint32_t n_tiles, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, int mode, const LaunchProbe* probe);
int rtu_launch_feat19(const KernelArgs& args, uint32_t n_tiles, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, int mode, const LaunchProbe* probe);
int rtu_launch_feat26(const KernelArgs& args, uint32_t n_tiles, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, int mode, const LaunchProbe* probe);
int rtu_launch_feat27(const KernelArgs& args, uint32_t n_tiles, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, int mode, const LaunchProbe* probe);
int rtu_launch_feat20(const KernelArgs& args, uint32_t n_tiles, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, int mode, const LaunchProbe* probe);
int rtu_launch_feat21(const KernelArgs& args, uint32_t n_tiles, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, int mode, const LaunchProbe* probe);

int rtu_launch_frame(const KernelArgs& args, uint32_t n_tiles, uint32_t bvh_stack_needed, int stats, hipStream_t stream, int mode, const LaunchProbe* probe) {
    // textured scenes, sampled frames and batches of frames run their own instantiations: the others carry no
    // uvw, sample nothing and draw nothing.
    const bool ref = stats == 1;
    if (mode != RTU_LAUNCH_ALL) {
        if (stats == 2) return args.scene.textured ? rtu_launch_feat27(args, n_tiles, bvh_stack_needed, false, stream, mode, probe)
                                                   : rtu_launch_feat26(args, n_tiles, bvh_stack_needed, false, stream, mode, probe);
        if (args.scene.textured) return rtu_launch_feat11(args, n_tiles, bvh_stack_needed, ref, stream, mode, probe);
        return rtu_launch_feat10(args, n_tiles, bvh_stack_needed, ref, stream, mode, probe);
    }
    const int feat = (args.scene.textured ? 1 : 0) | (args.sampling ? 2 : (args.frame_batch ? 4 : 0));
    if (stats == 2) {  // touched-bytes mode: one frame, frames in flight, or a batch of samples
        switch (feat) {
            case 0: return rtu_launch_feat16(args, n_tiles, bvh_stack_needed, false, stream, mode, probe);
            case 1: return rtu_launch_feat17(args, n_tiles, bvh_stack_needed, false, stream, mode, probe);
            case 2: return rtu_launch_feat18(args, n_tiles, bvh_stack_needed, false, stream, mode, probe);
            case 3: return rtu_launch_feat19(args, n_tiles, bvh_stack_needed, false, stream, mode, probe);
            case 4: return rtu_launch_feat20(args, n_tiles, bvh_stack_needed, false, stream, mode, probe);
            case 5: return rtu_launch_feat21(args, n_tiles, bvh_stack_needed, false, stream, mode, probe);
            default: return (int)hipErrorInvalidValue;
        }
    }
    switch (feat) {
        case 0: return rtu_launch_feat0(args, n_tiles, bvh_stack_needed, ref, stream, mode, probe);
        case 1: return rtu_launch_feat1(args, n_tiles, bvh_stack_needed, ref, stream, mode, probe);
        case 2: return rtu_launch_feat2(args, n_tiles, bvh_stack_needed, ref, stream, mode, probe);
        case 3: return rtu_launch_feat3(args, n_tiles, bvh_stack_needed, ref, stream, mode, probe);
        case 4: return rtu_launch_feat4(args, n_tiles, bvh_stack_needed, ref, stream, mode, probe);
        default: return rtu_launch_feat5(args, n_tiles, bvh_stack_needed, ref, stream, mode, probe);
    }
}

int rtu_launch_rays0(const KernelArgs& args, const float4* rays, uint32_t n, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, const LaunchProbe* probe);
int rtu_launch_rays1(const KernelArgs& args, const float4* rays, uint32_t n, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, const LaunchProbe* probe);

int rtu_launch_ray_batch(const KernelArgs& args, const float4* rays, uint32_t n, uint32_t bvh_stack_needed, bool stats, hipStream_t stream, const LaunchProbe* probe) {
    if (args.sampling || args.frame_batch) return (int)hipErrorInvalidValue;  // feature sets 0 and 1 only
    return args.scene.textured ? rtu_launch_rays1(args, rays, n, bvh_stack_needed, stats, stream, probe)
                               : rtu_launch_rays0(args, rays, n, bvh_stack_needed, stats, stream, probe);
}

int rtu_launch_gi_final(const KernelArgs& args, hipStream_t stream) {
    hipLaunchKernelGGL(k_gi_final, dim3((args.gi_total + 255u) / 256u), dim3(256), 0, stream, args);
    return (int)hipGetLastError();
}
