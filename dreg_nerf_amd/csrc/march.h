// Device code shared by the ray marchers over a NeRF block's occupancy grid (gfx950, wave64): the surface-visibility labels of
// visibility.hip and the volume renderer of render.hip.  Both march one ray per lane, 64 rays per wave, through the same three steps:
//   * march_advance   — the lane's next lattice sample t_mid = t_min + (n + 1/2) dt that lies in an occupied cell of the binary grid
//                       (nerfacc 0.3.5's marching rule; empty cells, and with the coarse bits empty 4^3 blocks, are skipped to their exit);
//   * march_density   — the density of the wave's 64 samples: hash-grid gather per lane, then the 32 -> 64 -> 16 MLP on fp16 MFMA
//                       through LDS (both stated in csrc/ngp_field.h, which the dense query of ngp.hip calls as well);
//   * the caller's own use of sigma (labels there, compositing here).
#pragma once
#include "ngp_field.h"   // NgpLevels, NGP_XRS / NGP_HRS, wave_sync, the level gather and the density MLP

// The occupancy grid a march walks: binary uint8 [rx,ry,rz] over the roi aabb, and optionally one bit per 4^3 block of it held in LDS (sCoarse).
struct MarchGrid {
    const uint8_t* binary;
    const uint32_t* sCoarse;     // null: no coarse bits
    float roi[6], roi_ext[3];
    int rdim[3], ry, rz, cy, cz;
};

// Rounding allowance, in position, of a lattice sample's distance to a cell face on one axis.  A sample's fp32 coordinate
// x = fl(o + fl(t d)) with t = fl(t_min + fl((n + 1/2) dt)) is within 2^-24 (|o| + 6 |t d|) of the exact line, and its cell index
// floor(fl(fl(fl(x - lo) / ext) res)) moves it by at most 4 * 2^-24 ext more; |t d| <= |o| + m inside the roi, where m is the larger of
// |lo| and |hi|, and ext <= 2 m.  That bounds the current sample, the face and any later sample of the same cell together by
// 2^-24 (7 |o| + 14 m) each; the allowance is 2^-19 (|o| + m), above twice that.
__device__ __forceinline__ float march_face_slack(float o_k, float roi_lo_k, float roi_hi_k)
{
    return 0x1p-19f * (fabsf(o_k) + fmaxf(fabsf(roi_lo_k), fabsf(roi_hi_k)));
}
// Lattice points a ray may pass over between a sample at distance `gap` (>= 0, along one axis with direction component d_k != 0) from the
// face through which it leaves its empty cell, and that face: those whose fp32 position is still inside the cell WHATEVER the rounding, i.e.
// at most (gap - slack) / (|d_k| dt) steps ahead, less 2^-20 relative for the roundings of the two quotients.  (The constant allowance this
// replaces, 1e-3 of a step, is less than the rounding of x once |d_k| dt is below ~1e-4: nearly axis-parallel rays at dt = 1e-3 lost a sample.)
__device__ __forceinline__ float march_steps_to_face(float gap, float slack, float d_k, float dt)
{
    return fmaxf(gap - slack, 0.f) / (fabsf(d_k) * dt) * (1.f - 0x1p-20f);
}

// Advance one live ray (active) to its next lattice sample inside an occupied cell, at most `guard_max` cells per call.  On return:
// true = a sample at t_mid = *tm_out, position x;  false with active cleared = the ray has left [t_min, t_max);
// false with active set = the guard ran out inside empty space (the caller continues on its next pass).  A point outside the roi is
// unoccupied; an inside point's cell is floor(u * res) clamped to the grid.
// CONTRACT of the skip: from a sample in an empty cell (or, with the coarse bits, an empty 4^3 block) the ray passes over only lattice points
// whose fp32 position, evaluated exactly as this loop evaluates it, lies in that same cell: march_steps_to_face keeps the rounding allowance
// of march_face_slack away from the exit face on every axis.  Every point passed over would therefore have been found empty, so the samples
// returned are the ones stepping through every lattice point returns — with or without coarse bits, for any direction and step
// (tests/test_hip_march_exact.py).  Within the allowance of the face the ray steps one lattice point at a time.
__device__ __forceinline__ bool march_advance(const MarchGrid& g, const float (&o)[3], const float (&d)[3], float tmin, float tmax, float dt, int& n, bool& active, float (&x)[3], float* tm_out, int guard_max)
{
    for (int guard = 0; active && guard < guard_max; ++guard) {
        const float tm = tmin + ((float)n + 0.5f) * dt;
        if (tm >= tmax) { active = false; break; }
        float u[3];
        bool inside = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) { x[k] = o[k] + tm * d[k]; u[k] = (x[k] - g.roi[k]) / g.roi_ext[k]; inside = inside && u[k] >= 0.f && u[k] <= 1.f; }
        int ci[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) ci[k] = min(max((int)floorf(u[k] * (float)g.rdim[k]), 0), g.rdim[k] - 1);
        // an empty COARSE cell holds no occupied fine cell: skip to ITS exit
        int cell_lo[3] = {ci[0], ci[1], ci[2]}, cell_w = 1;
        bool occ = false;
        if (inside) {
            bool coarse_empty = false;
            if (g.sCoarse) {
                const int b = ((ci[0] >> 2) * g.cy + (ci[1] >> 2)) * g.cz + (ci[2] >> 2);
                coarse_empty = ((g.sCoarse[b >> 5] >> (b & 31)) & 1u) == 0u;
            }
            if (coarse_empty) { cell_lo[0] = ci[0] & ~3; cell_lo[1] = ci[1] & ~3; cell_lo[2] = ci[2] & ~3; cell_w = 4; }
            else occ = g.binary[((long)ci[0] * g.ry + ci[1]) * g.rz + ci[2]] != 0;
        }
        if (occ) { if (tm_out) *tm_out = tm; return true; }
        float steps = 1e9f;                                                            // lattice steps to the exit face, rounding allowed for
        if (inside) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (d[k] != 0.f) {
                    const int hi = min(cell_lo[k] + cell_w, g.rdim[k]);                // (a ragged last coarse cell ends at the grid's face)
                    const float face = g.roi[k] + (float)(d[k] > 0.f ? hi : cell_lo[k]) * g.roi_ext[k] / (float)g.rdim[k];
                    steps = fminf(steps, march_steps_to_face(fabsf(face - x[k]), march_face_slack(o[k], g.roi[k], g.roi[3 + k]), d[k], dt));
                }
            }
        } else steps = 0.f;
        n += 1 + max((int)floorf(steps), 0);
    }
    return false;
}

// Density of the wave's 64 samples (lane = sample; lanes without one, have == false, take a zero row).  Returns whether x lies strictly
// inside the model aabb (outside: sigma = 0); sOut[lane] = fp16(h0), the density logit (sigma = exp(h0 - 1)).  FEAT: the 15 geometry
// features h1..h15 are also left in LDS, fp16, in columns 16..30 of the sample's row of sX (the colour net's input row: render.hip).
// sX: 64 rows of NGP_XRS bytes, sH: 64 rows of NGP_HRS bytes (apart from sX), sOut: 64 floats — all of this wave only.
template <bool FEAT>
__device__ __forceinline__ bool march_density(bool have, const float (&x)[3], const float* model, const NgpLevels& lv, const _Float16* table,
                                              const NgpDensityW& w, char* sX, char* sH, float* sOut, int lane)
{
    const int fr = lane & 15, kg = lane >> 4;
    float u[3];
    const bool inside_m = ngp_unit_cube(x, model, model + 3, 0, u) && have;
#pragma unroll 2
    for (int l = 0; l < 16; ++l) {
        float f0 = 0.f, f1 = 0.f;
        if (have) ngp_level_features(table, lv, l, u, f0, f1);
        _Float16* xr = reinterpret_cast<_Float16*>(sX + lane * NGP_XRS);
        xr[2 * l] = (_Float16)f0; xr[2 * l + 1] = (_Float16)f1;
    }
    ngp_density_mlp(w, sX, sH, lane, [&](int rb, const f32x4_t& ov) {      // ov[r] = output fr of sample rb*16 + kg*4 + r
        if (fr == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) sOut[rb * 16 + kg * 4 + r] = (float)(_Float16)ov[r];
        } else if (FEAT) {
#pragma unroll
            for (int r = 0; r < 4; ++r) reinterpret_cast<_Float16*>(sX + (rb * 16 + kg * 4 + r) * NGP_XRS)[15 + fr] = (_Float16)ov[r];
        }
    });
    wave_sync();
    return inside_m;
}

// ---- the renderer's per-ray setup and colour net, shared by the forward (render.hip) and the training backward (render_train.hip), which
// re-marches every ray and must reproduce the forward's survivors and colours exactly.

// Slab test of a ray against the scene aabb (t_min clamped at 0), then the near / far planes.  Returns whether the ray hits the aabb; the
// caller still checks t_min < t_max (after its jitter, if any).
__device__ __forceinline__ bool render_ray_interval(const float (&o)[3], const float (&d)[3], const float* scene, float near_plane, float far_plane,
                                                    float& tmin, float& tmax)
{
    float near = -1e30f, far = 1e30f;
    bool hit = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (d[k] == 0.f) { hit = hit && o[k] >= scene[k] && o[k] <= scene[3 + k]; continue; }   // parallel to the slab
        const float id = 1.f / d[k];
        float t0 = (scene[k] - o[k]) * id, t1 = (scene[3 + k] - o[k]) * id;
        if (t0 > t1) { const float tt = t0; t0 = t1; t1 = tt; }
        near = fmaxf(near, t0); far = fminf(far, t1);
    }
    hit = hit && near <= far && far > 0.f;
    tmin = fmaxf(fmaxf(near, 0.f), near_plane);
    tmax = fminf(far, far_plane);
    return hit;
}

// fp16 SH4(d) of a unit direction, two per word: the first 16 inputs of the colour net.
__device__ __forceinline__ void render_sh4_f16(const float (&d)[3], uint32_t (&sh2)[8])
{
    typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
    const float x = d[0], y = d[1], z = d[2];
    const float xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
    const float sh[16] = {0.28209479177387814f, -0.48860251190291987f * y, 0.48860251190291987f * z, -0.48860251190291987f * x,
                          1.0925484305920792f * xy, -1.0925484305920792f * yz, 0.94617469575755997f * z2 - 0.31539156525251999f,
                          -1.0925484305920792f * xz, 0.54627421529603959f * x2 - 0.54627421529603959f * y2,
                          0.59004358992664352f * y * (-3.0f * x2 + y2), 2.8906114426405538f * xy * z,
                          0.45704579946446572f * y * (1.0f - 5.0f * z2), 0.3731763325901154f * z * (5.0f * z2 - 3.0f),
                          0.45704579946446572f * x * (1.0f - 5.0f * z2), 1.4453057213202769f * z * (x2 - y2),
                          0.59004358992664352f * x * (-x2 + 3.0f * y2)};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const f16x2_t p = {(_Float16)sh[2 * j], (_Float16)sh[2 * j + 1]};
        sh2[j] = __builtin_bit_cast(uint32_t, p);
    }
}

// The colour net of the wave's 64 rows of sX (fp16 SH4(d) | 15 features | 1) -> relu 64 (sH1) -> relu 64 (sH2) -> 3 (sO[row*4 + ch], fp32 pre-
// activation; channel 3 is padding), the arithmetic of ngp_rgb_kernel.  sH1 may equal sH2 (the forward's in-place second layer: a 16-row block
// is read into registers in full before its outputs are written); the backward keeps both layers.  cw1f / cw3f: the first / last layer as
// MFMA operands (fp16 [64][32] rows cb*16 + fr, [16][64] row fr), cw2: fp16 [64][64] in memory.
__device__ __forceinline__ void march_color(char* sX, char* sH1, char* sH2, float* sO, const f16x8_t (&cw1f)[4], const _Float16* cw2,
                                            const f16x8_t (&cw3f)[2], int lane)
{
    typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
    const int fr = lane & 15, kg = lane >> 4;
    wave_sync();
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        const f16x8_t af = *reinterpret_cast<const f16x8_t*>(sX + (rb * 16 + fr) * NGP_XRS + kg * 16);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const f32x4_t v = __builtin_amdgcn_mfma_f32_16x16x32_f16(cw1f[cb], af, (f32x4_t){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            const f16x2_t z = {(_Float16)0.f, (_Float16)0.f};
            f16x2_t p = {(_Float16)v[0], (_Float16)v[1]}, q = {(_Float16)v[2], (_Float16)v[3]};
            p = __builtin_elementwise_max(p, z);
            q = __builtin_elementwise_max(q, z);
            uint32_t* dst = reinterpret_cast<uint32_t*>(sH1 + (rb * 16 + fr) * NGP_HRS + (cb * 16 + kg * 4) * 2);
            dst[0] = __builtin_bit_cast(uint32_t, p); dst[1] = __builtin_bit_cast(uint32_t, q);
        }
    }
    wave_sync();
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        f16x8_t af[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) af[kb] = *reinterpret_cast<const f16x8_t*>(sH1 + (rb * 16 + fr) * NGP_HRS + (kb * 32 + kg * 8) * 2);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            f32x4_t h = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
                h = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8_t*>(cw2 + (cb * 16 + fr) * 64 + kb * 32 + kg * 8), af[kb], h, 0, 0, 0);
            const f16x2_t z = {(_Float16)0.f, (_Float16)0.f};
            f16x2_t p = {(_Float16)h[0], (_Float16)h[1]}, q = {(_Float16)h[2], (_Float16)h[3]};
            p = __builtin_elementwise_max(p, z);
            q = __builtin_elementwise_max(q, z);
            uint32_t* dst = reinterpret_cast<uint32_t*>(sH2 + (rb * 16 + fr) * NGP_HRS + (cb * 16 + kg * 4) * 2);
            dst[0] = __builtin_bit_cast(uint32_t, p); dst[1] = __builtin_bit_cast(uint32_t, q);
        }
    }
    wave_sync();
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        f32x4_t ov = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
            ov = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8_t*>(sH2 + (rb * 16 + fr) * NGP_HRS + (kb * 32 + kg * 8) * 2), cw3f[kb], ov, 0, 0, 0);
        if (fr < 4) {        // channel fr of samples rb*16 + kg*4 + r (channel 3 is padding: written, never read)
#pragma unroll
            for (int r = 0; r < 4; ++r) sO[(rb * 16 + kg * 4 + r) * 4 + fr] = ov[r];
        }
    }
    wave_sync();
}

// fp16 colour channel of a pre-activation (the forward's sigmoid, rounded as tcnn's fp16 output)
__device__ __forceinline__ float march_sigmoid_f16(float pre)
{
    const float hv = (float)(_Float16)pre;
    return (float)(_Float16)__builtin_amdgcn_rcpf(1.f + __expf(-hv));
}
