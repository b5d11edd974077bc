// The density field of a NeRF block (Instant-NGP), stated once for every kernel that evaluates it (gfx950, wave64): the 16-level hash-grid
// encoding of a point (NGPradianceField.query_density, conerf/radiance_fields/ngp.py:148-176: HashGrid L=16 F=2) and the 32 -> 64 -> 16
// density MLP on fp16 MFMA (16x16x32) through LDS.  The dense query (ngp.hip), the ray marchers (march.h: visibility.hip, render.hip) and
// the training backward (render_train.hip), which re-marches every ray, must agree bit for bit: they all call the functions below.
// The kernels that differentiate the field by position (ngp_grad.hip, field_input_grad.hip) share ngp_relu_mask and ngp_encoding_dx.
// Table and weights are fp16, trilinear interpolation in fp32 rounded to fp16, layer inputs fp16, accumulation fp32.
#pragma once
#include "common.h"

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

// LDS row strides of the MLP tiles (bytes): 32 fp16 inputs / 64 fp16 hidden units per sample, padded against bank conflicts
constexpr int NGP_XRS = 32 * 2 + 16, NGP_HRS = 64 * 2 + 16;

struct NgpLevels {
    uint32_t offset[16];   // first entry of the level (entries of 2 features)
    uint32_t size[16];     // entries in the level
    uint32_t res[16];
    float scale[16];
    uint32_t hashed[16];
};
// from the five 16-entry host arrays of the C ABI (as produced by dreg_ngp_level_table)
static inline void ngp_fill_levels(NgpLevels& lv, const uint32_t* offset, const uint32_t* size, const uint32_t* res, const float* scale, const uint32_t* hashed)
{
    for (int l = 0; l < 16; ++l) { lv.offset[l] = offset[l]; lv.size[l] = size[l]; lv.res[l] = res[l]; lv.scale[l] = scale[l]; lv.hashed[l] = hashed[l]; }
}

__device__ __forceinline__ uint32_t grid_index(uint32_t x, uint32_t y, uint32_t z, uint32_t res, uint32_t size, uint32_t hashed) {
    uint32_t idx = hashed ? (x ^ (y * 2654435761u) ^ (z * 805459861u)) : (x + y * res + z * res * res);
    return idx % size;
}

__device__ __forceinline__ f16x8_t ldsfrag(const char* base, int rs, int row, int k0) {
    return *reinterpret_cast<const f16x8_t*>(base + row * rs + k0 * 2);
}

// Every wave owns its 64 points and its own slice of LDS (sX / sH of wave w): what one layer writes is read back by the SAME wave.  LDS
// instructions of a wave execute in issue order, so no workgroup barrier is needed between the layers — only the compiler must not
// move the reads above the writes.  (Six __syncthreads per direction kept the four waves of a workgroup in lockstep.)
__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

// Hidden activations go back to LDS between the layers.  The products are formed TRANSPOSED (weights as the MFMA's first operand), so a
// lane holds four consecutive hidden units of one point: one 8-byte LDS write of four fp16 instead of four 2-byte writes (the layers
// are 16-64 MFMAs each; 64 scalar LDS writes per lane and layer were most of the kernel).  Same products, same sums: bit-identical.
__device__ __forceinline__ void store_relu4(char* sH, int row_stride, int point, int hidden, const f32x4_t& v)
{
    typedef __attribute__((ext_vector_type(4))) _Float16 f16x4_t;
    const f16x4_t h = {(_Float16)fmaxf(v[0], 0.f), (_Float16)fmaxf(v[1], 0.f), (_Float16)fmaxf(v[2], 0.f), (_Float16)fmaxf(v[3], 0.f)};
    *reinterpret_cast<f16x4_t*>(sH + point * row_stride + hidden * 2) = h;
}

// The same with the ReLU on the packed-half VALU: round the four sums to fp16 first (round-to-nearest, as the plain cast), then ONE
// v_pk_max_f16 per pair — relu(rn(x)) == rn(relu(x)), so the stored bits are those of store_relu4.  (The library is built without
// packed-fp32 VALU instructions; packed fp16 ones are not affected: DESIGN.md, co-execution fault.)
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void store_relu4_pk(char* sH, int row_stride, int point, int hidden, const f32x4_t& v)
{
    typedef __attribute__((ext_vector_type(4))) _Float16 f16x4_t;
    const f16x2_t z = {(_Float16)0.f, (_Float16)0.f};
    f16x2_t a = {(_Float16)v[0], (_Float16)v[1]}, b = {(_Float16)v[2], (_Float16)v[3]};
    a = __builtin_elementwise_max(a, z);
    b = __builtin_elementwise_max(b, z);
    const f16x4_t h = {a[0], a[1], b[0], b[1]};
    *reinterpret_cast<f16x4_t*>(sH + point * row_stride + hidden * 2) = h;
}

// ------------------------------------------------------------------------------------------------ unit coordinates
// Unit-cube coordinates u (clamped to [0,1]) of the world position x in the aabb (lo, hi), and whether x lies strictly inside
// (ngp.py:157-167; outside, the callers set the density to 0).
__device__ __forceinline__ bool ngp_unit_cube(const float (&x)[3], const float* lo, const float* hi, int contract, float (&u)[3])
{
    bool inside = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) u[c] = (x[c] - lo[c]) / (hi[c] - lo[c]);
    if (contract) {
        // contract_to_unisphere (conerf/radiance_fields/ngp.py:41-63): the aabb maps to [-1,1]^3, points of norm > 1 are pulled
        // onto the shell (2 - 1/|x|) x/|x| of radius < 2, and [-2,2]^3 maps to [0,1]^3
        float v[3], m2 = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) { v[c] = u[c] * 2.f - 1.f; m2 += v[c] * v[c]; }
        const float mag = sqrtf(m2);
        if (mag > 1.f) {
            const float sc = (2.f - 1.f / mag) / mag;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] *= sc;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] = v[c] / 4.f + 0.5f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        inside = inside && (u[c] > 0.f) && (u[c] < 1.f);
        u[c] = fminf(fmaxf(u[c], 0.f), 1.f);
    }
    return inside;
}

// ------------------------------------------------------------------------------------------------ hash-grid level
// The 8 corners of level l around unit coordinates u: hook(e, wt) is called per corner with e = the corner's first fp16 element within
// the level (2 * entry: add 2 * lv.offset[l] for the whole table) and its trilinear weight.  hook is a lambda, inlined: no indirect call.
template <typename Hook>
__device__ __forceinline__ void ngp_level_corners(const NgpLevels& lv, int l, const float (&u)[3], Hook&& hook)
{
    const float sc = lv.scale[l];
    const uint32_t res = lv.res[l], size = lv.size[l], hashed = lv.hashed[l];
    float pos[3], w[3];
    uint32_t g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { pos[c] = u[c] * sc + 0.5f; const float fl = floorf(pos[c]); g[c] = (uint32_t)fl; w[c] = pos[c] - fl; }
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
        const uint32_t cx = g[0] + (corner & 1), cy = g[1] + ((corner >> 1) & 1), cz = g[2] + ((corner >> 2) & 1);
        const float wt = ((corner & 1) ? w[0] : 1.f - w[0]) * ((corner & 2) ? w[1] : 1.f - w[1]) * ((corner & 4) ? w[2] : 1.f - w[2]);
        hook((size_t)grid_index(cx, cy, cz, res, size, hashed) * 2, wt);
    }
}
// one corner's share of the level's two features: a 4-byte gather of the fp16 pair at tl + e
__device__ __forceinline__ void ngp_corner_accumulate(const _Float16* tl, size_t e, float wt, float& f0, float& f1)
{
    union { uint32_t u32; _Float16 h[2]; } cv;
    cv.u32 = *reinterpret_cast<const uint32_t*>(tl + e);
    f0 += wt * (float)cv.h[0]; f1 += wt * (float)cv.h[1];
}
// trilinear interpolation of level l's two features at unit coordinates u (8 corner gathers of 4 bytes)
__device__ __forceinline__ void ngp_level_features(const _Float16* __restrict__ table, const NgpLevels& lv, int l, const float (&u)[3], float& f0, float& f1)
{
    const _Float16* tl = table + (size_t)lv.offset[l] * 2;
    f0 = 0.f; f1 = 0.f;
    ngp_level_corners(lv, l, u, [&](size_t e, float wt) { ngp_corner_accumulate(tl, e, wt, f0, f1); });
}

// The encoding's derivative by position for a row f[32] of gradients by the 32 encoded features (ngp_grad.hip, field_input_grad.hip):
//   du_c = sum_l scale_l sum_corners (s_c w_a w_b) (f[2l] t_0 + f[2l+1] t_1),   s_c = +-1 by the corner's side on axis c, w_a, w_b the trilinear
// weights of the other two axes, t the corner's two table entries.  The corner loop of every level runs again with a hook that accumulates the
// three derivatives: the same gathers as the forward, no atomics.  The caller scales by 1 / (hi_c - lo_c) and masks by its own rule.
__device__ __forceinline__ void ngp_encoding_dx(const _Float16* __restrict__ table, const NgpLevels& lv, const float (&u)[3], const float* f, float (&du)[3])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) du[c] = 0.f;
#pragma unroll 1
    for (int l = 0; l < 16; ++l) {
        const float f0 = f[2 * l], f1 = f[2 * l + 1];
        const float sc = lv.scale[l];
        float w[3];                                      // the trilinear weights as ngp_level_corners forms them
#pragma unroll
        for (int c = 0; c < 3; ++c) { const float pos = u[c] * sc + 0.5f; w[c] = pos - floorf(pos); }
        const _Float16* tl = table + (size_t)lv.offset[l] * 2;
        float D[3] = {0.f, 0.f, 0.f};
        int corner = 0;                                  // ngp_level_corners calls the hook for corner 0..7 in order (unrolled: a constant)
        ngp_level_corners(lv, l, u, [&](size_t e, float) {
            union { uint32_t u32; _Float16 h[2]; } cv;
            cv.u32 = *reinterpret_cast<const uint32_t*>(tl + e);
            const float v = f0 * (float)cv.h[0] + f1 * (float)cv.h[1];
            const float wx = (corner & 1) ? w[0] : 1.f - w[0], wy = (corner & 2) ? w[1] : 1.f - w[1], wz = (corner & 4) ? w[2] : 1.f - w[2];
            const float a0 = (wy * wz) * v, a1 = (wx * wz) * v, a2 = (wx * wy) * v;
            D[0] += (corner & 1) ? a0 : -a0;
            D[1] += (corner & 2) ? a1 : -a1;
            D[2] += (corner & 4) ? a2 : -a2;
            ++corner;
        });
#pragma unroll
        for (int c = 0; c < 3; ++c) du[c] += sc * D[c];
    }
}

// ------------------------------------------------------------------------------------------------ density MLP
// The ReLU mask of a lane's own row of a hidden tile (64 fp16 units, stride NGP_HRS): bit j = the stored activation j is > 0.
__device__ __forceinline__ unsigned long long ngp_relu_mask(const char* sH, int lane)
{
    unsigned long long mask = 0ull;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const f16x8_t h = ldsfrag(sH, NGP_HRS, lane, k * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) mask |= (h[j] > (_Float16)0.f) ? (1ull << (k * 8 + j)) : 0ull;
    }
    return mask;
}

// The density MLP's weights as MFMA operands, held in registers: w1 fp16 [64][32], w2 fp16 [16][64].
struct NgpDensityW { f16x8_t w1f[4], w2f[2]; };
__device__ __forceinline__ void ngp_load_density_w(NgpDensityW& w, const _Float16* w1, const _Float16* w2, int lane)
{
    const int fr = lane & 15, kg = lane >> 4;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) w.w1f[cb] = *reinterpret_cast<const f16x8_t*>(w1 + (cb * 16 + fr) * 32 + kg * 8);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) w.w2f[kb] = *reinterpret_cast<const f16x8_t*>(w2 + fr * 64 + kb * 32 + kg * 8);
}

// The 32 -> 64 -> 16 net over the wave's 64 samples: input rows in sX (64 rows of NGP_XRS bytes, 32 fp16 each, written by this wave
// before the call) -> fp32 sums -> ReLU, fp16 rows in sH (64 rows of NGP_HRS bytes) -> second layer.  epi(rb, ov) receives, for each
// block rb of 16 samples, ov[r] = output (lane & 15) of sample rb*16 + (lane >> 4)*4 + r, fp32.
// Aliasing: sX may lie INSIDE sH (ngp_density_kernel keeps one tile per wave) — every first-layer sum is formed before the first store to
// sH — but then epi must not write to sX.  An epi that writes sX (march_density<FEAT>) needs sX and sH apart.  Buffers that epi fills for
// the caller need the caller's wave_sync() before they are read.
template <typename Epi>
__device__ __forceinline__ void ngp_density_mlp(const NgpDensityW& w, const char* sX, char* sH, int lane, Epi&& epi)
{
    const int fr = lane & 15, kg = lane >> 4;
    wave_sync();
    f32x4_t acc[4][4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        const f16x8_t af = ldsfrag(sX, NGP_XRS, rb * 16 + fr, kg * 8);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.w1f[cb], af, (f32x4_t){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    }
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) store_relu4(sH, NGP_HRS, rb * 16 + fr, cb * 16 + kg * 4, acc[rb][cb]);   // hidden units cb*16 + kg*4 .. +3 of sample rb*16 + fr
    wave_sync();
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        f32x4_t ov = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) ov = __builtin_amdgcn_mfma_f32_16x16x32_f16(ldsfrag(sH, NGP_HRS, rb * 16 + fr, kb * 32 + kg * 8), w.w2f[kb], ov, 0, 0, 0);
        epi(rb, ov);
    }
}

// ------------------------------------------------------------------------------------------------ colour MLP, shared directions, 16-point tiles
// The colour net's weights as MFMA operands, held in registers across tiles and directions: w1 fp16 [64][32], w2 fp16 [64][64], w3 fp16 [16][64].
struct NgpColorW { f16x8_t w1f[4], w2f[4][2], w3f[2]; };
__device__ __forceinline__ void ngp_load_color_w(NgpColorW& w, const _Float16* w1, const _Float16* w2, const _Float16* w3, int lane)
{
    const int fr = lane & 15, kg = lane >> 4;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        w.w1f[cb] = *reinterpret_cast<const f16x8_t*>(w1 + (cb * 16 + fr) * 32 + kg * 8);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) w.w2f[cb][kb] = *reinterpret_cast<const f16x8_t*>(w2 + (cb * 16 + fr) * 64 + kb * 32 + kg * 8);
    }
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) w.w3f[kb] = *reinterpret_cast<const f16x8_t*>(w3 + fr * 64 + kb * 32 + kg * 8);
}

// The per-tile body of the chunked colour kernel (ngp_rgb_chunks_kernel of ngp.hip; the merged voxel grid of scene_grid.hip calls it too, so
// the two agree bit for bit by construction).  On entry the first 16 rows of sH (stride NGP_XRS) hold X = (0 x16 | feat[1..15] | 1) of the
// tile's 16 points, written by this wave; sH is one 16 x 64 fp16 tile (stride NGP_HRS), sO 16 x 4 floats.  ones: 1 in K columns 0 and 1 of the
// kg == 0 lanes, 0 elsewhere; biaspk: uint32 [ndir][64] = fp16 (hi | lo << 16) of the direction's bias c_k[j] (ngp_dir_bias_kernel).  Returns,
// in lanes 0..47 = (point lane / 3, channel lane % 3), the SUM over the directions of fp16(sigmoid(fp16(pre-activation))); the caller scales by
// 1 / ndir.  A point's row depends on that row alone.  The caller's wave_sync() follows before the tile or sO is rewritten.
__device__ __forceinline__ float ngp_rgb_tile(const NgpColorW& w, const f16x8_t& ones, const uint32_t* __restrict__ biaspk, int ndir, char* sH, float* sO, int lane)
{
    constexpr int XRS = NGP_XRS, HRS = NGP_HRS;
    const int fr = lane & 15, kg = lane >> 4;
    const int opt = lane / 3, och = lane - opt * 3;                  // dense output role: lanes 0..47 = (point, channel) of the tile
    wave_sync();
    f32x4_t base[4];
    {
        const f16x8_t af = ldsfrag(sH, XRS, fr, kg * 8);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) base[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.w1f[cb], af, (f32x4_t){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    }
    float sum = 0.f;
#pragma unroll 1
    for (int k = 0; k < ndir; ++k) {
        f16x8_t bfr[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const uint32_t pk = kg == 0 ? biaspk[k * 64 + cb * 16 + fr] : 0u;
            typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
            bfr[cb] = __builtin_bit_cast(f16x8_t, (u32x4_t){pk, 0u, 0u, 0u});
        }
        wave_sync();
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
            store_relu4_pk(sH, HRS, fr, cb * 16 + kg * 4, __builtin_amdgcn_mfma_f32_16x16x32_f16(bfr[cb], ones, base[cb], 0, 0, 0));
        wave_sync();
        f16x8_t af[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) af[kb] = ldsfrag(sH, HRS, fr, kb * 32 + kg * 8);
        f32x4_t h[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            h[cb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) h[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.w2f[cb][kb], af[kb], h[cb], 0, 0, 0);
        }
        wave_sync();                                  // every lane has read its layer-1 fragments: the tile may be overwritten
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) store_relu4_pk(sH, HRS, fr, cb * 16 + kg * 4, h[cb]);
        wave_sync();
        f32x4_t o = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) o = __builtin_amdgcn_mfma_f32_16x16x32_f16(ldsfrag(sH, HRS, fr, kb * 32 + kg * 8), w.w3f[kb], o, 0, 0, 0);
        if (fr < 4) {
#pragma unroll
            for (int r = 0; r < 4; ++r) sO[(kg * 4 + r) * 4 + fr] = o[r];
        }
        wave_sync();
        const float hv = (float)(_Float16)sO[(lane < 48 ? opt : 0) * 4 + och];
        sum += (float)(_Float16)__builtin_amdgcn_rcpf(1.f + __expf(-hv));
    }
    return sum;
}
