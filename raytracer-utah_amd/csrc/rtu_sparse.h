// rtu_sparse.h — the arithmetic of sparse sessions (include/rtu_render.h "Sparse sessions"), host + device, and the launch interface of
// its kernels (rtu_sparse.hip), called by rtu_capi_temporal.hip:
//   sp_owner   the pixel a B x B block shades in frame k, and the class of the block (which of the four block sizes of an image it has)
//   sp_ray     rtu_sparse_rays: that pixel's ray and key (camera_sample_ray of rtu_camrays.h) in the sample its block has reached
//   sp_fill    rtu_sparse_fill: the colour shown at a pixel that has neither a sample nor a usable history
// The sparse accumulator is tp_pixel<true, true, false, true> of rtu_temporal.h. Binary32, one rounding per operation: the translation
// units that include this header are compiled with -ffp-contract=off and IEEE divides and square roots, so the host forms and the
// kernels give the same bits.
#ifndef RTU_SPARSE_H_INCLUDED
#define RTU_SPARSE_H_INCLUDED

#include "rtu_camrays.h"
#include "rtu_temporal.h"

#define SP_MAX_BLOCK 4

inline int32_t sp_blocks(int32_t pixels, int32_t block) { return (pixels + (block - 1)) / block; }

// ---- 1. owners and rays ----------------------------------------------------------------------------------------------------------
// m of the four classes of blocks of a width x height image: class = (narrower than B) + 2 * (lower than B). A class the image has
// no block of gets B * B (never read; no division by zero).
inline void sp_class_sizes(int32_t width, int32_t height, int32_t B, uint32_t m[4]) {
    const uint32_t rw = (uint32_t)(width % B), rh = (uint32_t)(height % B), b = (uint32_t)B;
    m[0] = b * b;
    m[1] = rw ? rw * b : b * b;
    m[2] = rh ? b * rh : b * b;
    m[3] = (rw && rh) ? rw * rh : b * b;
}

// the owner (x, y) of block b = bx + sw * by in frame k: always inside the block and the image
RTU_HD void sp_owner(int32_t width, int32_t height, int32_t B, int32_t sw, uint32_t b, uint32_t k, int& x, int& y, int& cls) {
    const int32_t by = (int32_t)(b / (uint32_t)sw), bx = (int32_t)(b - (uint32_t)by * (uint32_t)sw);
    const int32_t rw = width - B * bx, rh = height - B * by;
    const uint32_t bw = (uint32_t)(rw < B ? rw : B), bh = (uint32_t)(rh < B ? rh : B);
    const uint32_t m = bw * bh, full = (uint32_t)(B * B);
    const uint32_t j = k % m;
    const uint32_t t = m == full ? (j * (uint32_t)(2 * B - 1)) % m : j;  // M_B = 2 B - 1: 1, 3, 5, 7
    x = B * bx + (int32_t)(t % bw);
    y = B * by + (int32_t)(t / bw);
    cls = (rw < B ? 1 : 0) + (rh < B ? 2 : 0);
}

// what the rays of a frame need: the camera, and per class of blocks the sample s = (k div m) mod S with its pixel offsets
struct SpRays {
    CamSample c;  // (its ox, oy and sample are not read)
    float     ox[4], oy[4];
    uint32_t  sample[4];
    int32_t   block, sw;
    uint32_t  blocks, frame_index;
};

template <class SinCos>
RTU_HD void sp_ray(const SpRays& R, uint32_t b, SinCos sc, f3& org, f3& dir, uint32_t& key, uint32_t& owner) {
    int x, y, cls;
    sp_owner(R.c.width, R.c.height, R.block, R.sw, b, R.frame_index, x, y, cls);
    CamSample c = R.c;
    c.ox = R.ox[cls];
    c.oy = R.oy[cls];
    c.sample = R.sample[cls];
    camera_sample_ray(c, x, y, sc, org, dir, key);
    owner = (uint32_t)x + (uint32_t)R.c.width * (uint32_t)y;
}

// ---- 3. the fill -----------------------------------------------------------------------------------------------------------------
struct SpFill {
    int32_t width, height, block, sw, sh;
    float   sigma_plane, normal_min;
};

// The colour of hole pixel (x, y): hits (three float4 per pixel) and albedo the full-resolution guides, owner and rgbt one entry per
// block, cur the pixel as the accumulator left it (its z is kept). An owner outside the image is skipped.
RTU_HD float4 sp_fill(const SpFill& F, int x, int y, const float4* hits, const float4* albedo, const uint32_t* owner, const float4* rgbt, const float4& cur) {
    const size_t n = (size_t)F.width * (size_t)F.height;
    const size_t p = (size_t)y * (size_t)F.width + (size_t)x;
    union { float f; uint32_t u; } flags, node_p, node_q;
    const float4 hp0 = hits[3 * p], hp1 = hits[3 * p + 1], hp2 = hits[3 * p + 2];
    flags.f = hp0.z;
    node_p.f = hp0.y;
    const bool valid = (flags.u & RTU_RAY_HIT) != 0;
    const f3 d_p = dn_demod(albedo[p]);
    const f3 Pp = mk3(hp1.x, hp1.y, hp1.z), Np = mk3(hp2.x, hp2.y, hp2.z);
    const float plane_max = F.sigma_plane * hp0.x;
    f3 a1 = mk3(0.0f, 0.0f, 0.0f), a2 = mk3(0.0f, 0.0f, 0.0f);
    float w1 = 0.0f, w2 = 0.0f;
    const int bx = x / F.block, by = y / F.block;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int tx = bx + dx, ty = by + dy;
            if (tx < 0 || ty < 0 || tx >= F.sw || ty >= F.sh) continue;
            const size_t b = (size_t)ty * (size_t)F.sw + (size_t)tx;
            const size_t q = owner[b];
            const float4 c = rgbt[b];
            if (q >= n || !(tp_finite(c.x) && tp_finite(c.y) && tp_finite(c.z))) continue;
            const float4 hq0 = hits[3 * q];
            flags.f = hq0.z;
            if (((flags.u & RTU_RAY_HIT) != 0) != valid) continue;
            const int qy = (int)(q / (size_t)F.width), qx = (int)(q - (size_t)qy * (size_t)F.width);
            const float fdx = (float)(qx - x), fdy = (float)(qy - y);
            const float w = 1.0f / (1.0f + (fdx * fdx + fdy * fdy));
            const f3 d_q = dn_demod(albedo[q]);
            const f3 e = valid ? mk3(c.x / d_q.x, c.y / d_q.y, c.z / d_q.z) : mk3(c.x, c.y, c.z);
            const f3 ew = e * w;
            a2 = a2 + ew;
            w2 = w2 + w;
            if (!valid) continue;
            const float4 hq1 = hits[3 * q + 1], hq2 = hits[3 * q + 2];
            node_q.f = hq0.y;
            if (node_q.u != node_p.u) continue;
            if (!(dot3(Np, mk3(hq2.x, hq2.y, hq2.z)) >= F.normal_min)) continue;
            if (!(fabsf(dot3(Np, mk3(hq1.x, hq1.y, hq1.z) - Pp)) <= plane_max)) continue;
            a1 = a1 + ew;
            w1 = w1 + w;
        }
    const bool first = w1 > 0.0f;
    const f3 acc = first ? a1 : a2;
    const float ws = first ? w1 : w2;
    if (!(ws > 0.0f)) return make_float4(0.0f, 0.0f, 0.0f, cur.w);
    const f3 r = mk3(acc.x / ws, acc.y / ws, acc.z / ws);
    return valid ? make_float4(r.x * d_p.x, r.y * d_p.y, r.z * d_p.z, cur.w) : make_float4(r.x, r.y, r.z, cur.w);
}

// RTU_OK or RTU_ERR_ARG: the rules of RtuSparseDesc (include/rtu_render.h)
int rtu_sparse_check_desc(const RtuSparseDesc* d);

// Every launch function is asynchronous on `stream` and returns a hipError_t as int; pointers 16-byte (float4) or 4-byte aligned
// (owner, keys; hole: none) and descs checked by the caller.
// rays[2 * b ..], keys[b], owner[b] for every block b
int rtu_launch_sparse_rays(const SpRays& r, float4* rays, uint32_t* keys, uint32_t* owner, hipStream_t stream);
// rgbz[p] = sp_fill for every pixel p with hole[p] == 1; no other pixel is written
int rtu_launch_sparse_fill(const SpFill& f, const float4* hits, const float4* albedo, const uint32_t* owner, const float4* rgbt, const uint8_t* hole,
                           float4* rgbz, hipStream_t stream);

#endif
