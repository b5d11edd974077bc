// What the ray marchers over a NeRF block's occupancy grid share (gfx950, wave64): the surface-visibility labels (visibility.hip), the volume
// renderer (render.hip), its training backward (render_train.hip), the two-block and K-block renderers (render_pair.hip, render_scene.hip) and,
// for the block rules, the density field of registered blocks (scene_field.hip).  The marchers run one ray per lane, 64 rays per wave.  Stated
// here once:
//   * MarchBlock, march_fill_block, march_pass_bound — one block as a marcher reads it, and the ONE host function that validates and fills it
//                       from an entry point's arguments (nulls, grid dimensions, step, the 32,768-bit coarse rule, the scene diagonal and n_max);
//   * march_load_coarse, march_grid — the device set-up: coarse bits into LDS, the MarchGrid of a block;
//   * march_take      — one refill round: lanes without a ray take consecutive rays from a queue (MarchQueue) or a wave's own chunk (MarchChunk);
//   * march_advance   — the lane's next lattice sample t_mid = t_min + (n + 1/2) dt that lies in an occupied cell of the binary grid
//                       (nerfacc 0.3.5's marching rule; empty cells, and with the coarse bits empty 4^3 blocks, are skipped to their exit);
//   * march_density   — the density of the wave's 64 samples: hash-grid gather per lane, then the 32 -> 64 -> 16 MLP on fp16 MFMA
//                       through LDS (both stated in csrc/ngp_field.h, which the dense query of ngp.hip calls as well);
//   * march_sigma, march_composite, march_color_row — a renderer's sample step: sigma -> alpha -> survival -> T_all -> w, T_s with
//                       sigma_eff = omega sigma (omega = 1 in the one-block renderers), then the colour net's input row of a survivor;
//   * march_load_color_w, march_color, march_sigmoid_f16, render_ray_interval, render_sh4_f16 — the colour net and a renderer's ray set-up;
//   * the rules of REGISTERED blocks (render_pair.hip, render_scene.hip, scene_field.hip):
//     march_covered     — a block's own coverage of a point of its frame: inside the roi, the cell clamp(floor(u res), 0, res - 1) set;
//     march_cursor_ray  — a ray's cursor of one block: its interval, act, n_lim, the empty interval [1, 0) on a miss;
//     MarchAccum, march_accum_reset, march_sample_phase, march_write_ray, march_count_samples, march_report_overrun — the merged stream's
//                       accumulator, the sample phase of one block (density, march_composite, colour row, colour net, accumulation; the per-block
//                       share is the caller's), the common outputs of a ray and the kernel's tail (sample count, overrun report).
// The bit-for-bit contracts between the kernels (pair == render, scene(K = 2) == pair, train(jitter 0) == render, persistent == lock-step labels)
// rest on these being the same code.  Deliberately left apart:
//   * surface_visibility_kernel keeps its own advance loop: it is the reference the persistent form is tested against;
//   * vis_ray_setup keeps its own slab test: it has no parallel-axis case and no near / far, so its result on d[k] == 0 differs from
//     render_ray_interval's;
//   * visibility's sample update (best, stop_T) is another rule than march_composite and stays in visibility.hip;
//   * march_advance keeps its own copy of march_covered's lookup: there it is interleaved with the coarse-cell logic in the hot loop of four kernels;
//   * the two renderers of registered blocks stay two kernels (K = 2 through the LDS cursors of render_scene.hip measured 1.39 x the register
//     cursors of render_pair.hip); their block loops stay one non-unrolled body each that reads the block from the kernel-argument segment
//     (render_pair.hip's header says why), and where a cursor lives and how the next sample is picked is each kernel's own;
//   * the density phase of scene_field.hip is not march_density: it has no samples to refill and runs the gather not unrolled, at four waves;
//   * two kernels at the edge of their budgets keep one helper's body written out, and say so where they do: ngp_render_bwd_kernel fills its
//     MarchGrid itself (through march_grid it reserved more scratch), ngp_render_kernel its sample step (through march_composite / march_color_row
//     its training forward measured slower).  The arithmetic is the helpers'; the bit-for-bit tests between the kernels hold it there.
#pragma once
#include "ngp_field.h"   // NgpLevels, NGP_XRS / NGP_HRS, wave_sync, the level gather and the density MLP

// The occupancy grid a march walks: binary uint8 [rx,ry,rz] over the roi aabb, and optionally one bit per 4^3 block of it held in LDS (sCoarse).
struct MarchGrid {
    const uint8_t* binary;
    const uint32_t* sCoarse;     // null: no coarse bits
    float roi[6], roi_ext[3];
    int rdim[3], ry, rz, cy, cz;
};

// One block as a marcher reads it.  The kernel-argument structs of the four marchers begin with one; march_fill_block writes every field.
struct MarchBlock {
    const _Float16 *table, *w1, *w2;           // density net (fp16 inference copies of mlp_base.params)
    const _Float16 *cw1, *cw2, *cw3;           // colour net (color_mlp.params): [64][32], [64][64], [16][64]; null where the marcher has none
    NgpLevels lv;
    const uint8_t* binary;                     // [rx,ry,rz] occupancy over the roi aabb
    const uint32_t* coarse;                    // optional: one bit per 4^3 block of `binary` (dreg_occupancy_coarse_bits), <= 32,768 bits; null = none
    int rx, ry, rz, cx, cy, cz;                // c* = ceil(r* / 4)
    float roi[6], scene[6], model[6];
    float near, far, dt, alpha_thre;
    int n_max;                                 // samples per ray <= ceil(scene diagonal / dt) + 2; 0 where no scene interval is marched
};

// Validate and fill one block from an entry point's own arguments: DREG_OK, or DREG_EINVAL with nothing launched.  color: the marcher runs the
// colour net (cw1..cw3 required).  scene_interval: rays are marched through the scene aabb, so a degenerate aabb or a step too small to march
// it (diagonal / dt > 1e8) is rejected and n_max is set (<= 1e8 + 2: conversions of per-ray bounds to int cannot overflow).
static inline int march_fill_block(MarchBlock& b, const uint8_t* binary, int rx, int ry, int rz, const uint32_t* coarse_bits,
                                   const void* table, const void* w1, const void* w2, bool color, const void* cw1, const void* cw2, const void* cw3,
                                   const uint32_t* offset, const uint32_t* size, const uint32_t* res, const float* scale, const uint32_t* hashed,
                                   const float* roi_aabb, const float* scene_aabb, const float* model_aabb, float near_plane, float far_plane,
                                   float render_step_size, float alpha_thre, bool scene_interval)
{
    if (!binary || !table || !w1 || !w2 || (color && (!cw1 || !cw2 || !cw3)) || !offset || !size || !res || !scale || !hashed ||
        !roi_aabb || !scene_aabb || !model_aabb)
        return DREG_EINVAL;
    if (rx <= 0 || ry <= 0 || rz <= 0 || !(render_step_size > 0.f)) return DREG_EINVAL;
    b.table = (const _Float16*)table; b.w1 = (const _Float16*)w1; b.w2 = (const _Float16*)w2;
    b.cw1 = (const _Float16*)cw1; b.cw2 = (const _Float16*)cw2; b.cw3 = (const _Float16*)cw3;
    ngp_fill_levels(b.lv, offset, size, res, scale, hashed);
    for (int k = 0; k < 6; ++k) { b.roi[k] = roi_aabb[k]; b.scene[k] = scene_aabb[k]; b.model[k] = model_aabb[k]; }
    b.binary = binary; b.rx = rx; b.ry = ry; b.rz = rz;
    b.cx = (rx + 3) / 4; b.cy = (ry + 3) / 4; b.cz = (rz + 3) / 4;
    b.coarse = ((long)b.cx * b.cy * b.cz <= 32768) ? coarse_bits : nullptr;      // (the kernels keep a block's bits in 4 KB of LDS)
    b.near = near_plane; b.far = far_plane; b.dt = render_step_size; b.alpha_thre = alpha_thre;
    b.n_max = 0;
    if (scene_interval) {
        double diag = 0.0;
        for (int k = 0; k < 3; ++k) { const double e = (double)scene_aabb[3 + k] - (double)scene_aabb[k]; diag += e * e; }
        diag = __builtin_sqrt(diag);
        if (!(diag >= 0.0) || diag / render_step_size > 1e8) return DREG_EINVAL;
        b.n_max = (int)__builtin_ceil(diag / render_step_size) + 2;
    }
    return DREG_OK;
}

// Passes of a persistent march loop per wave, a safety net: every pass takes a ray, a sample or a lattice step.
static inline long march_pass_bound(long rays, double steps_per_ray)
{
    const double passes = (double)rays * steps_per_ray + 64.0;
    return passes > 1e15 ? (long)1e15 : (long)passes;
}

// The block's coarse bits into the one-wave workgroup's LDS (the caller's __syncthreads follows), and the grid a march of the block walks.
__device__ __forceinline__ void march_load_coarse(uint32_t* sCoarse, const MarchBlock& b, int lane)
{
    if (b.coarse != nullptr) {
        const int nw = (b.cx * b.cy * b.cz + 31) / 32;
        for (int i = lane; i < nw; i += 64) sCoarse[i] = b.coarse[i];
    }
}
__device__ __forceinline__ void march_grid(MarchGrid& g, const MarchBlock& b, const uint32_t* sCoarse)
{
    g.binary = b.binary; g.sCoarse = b.coarse != nullptr ? sCoarse : nullptr;
#pragma unroll
    for (int k = 0; k < 3; ++k) { g.roi[k] = b.roi[k]; g.roi[3 + k] = b.roi[3 + k]; g.roi_ext[k] = b.roi[3 + k] - b.roi[k]; }
    g.rdim[0] = b.rx; g.rdim[1] = b.ry; g.rdim[2] = b.rz; g.ry = b.ry; g.rz = b.rz; g.cy = b.cy; g.cz = b.cz;
}

// Where a refill round's rays come from: the first of popc(mask) consecutive ray indices, the same value in every lane.
struct MarchQueue {          // a counter in device memory shared by all waves: one atomic per wave and round
    unsigned long long* counter;
    __device__ __forceinline__ unsigned long long operator()(unsigned long long mask, int lane)
    {
        unsigned long long base = 0;
        const int leader = __ffsll((long long)mask) - 1;
        if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(mask));
        return __shfl(base, leader, 64);
    }
};
struct MarchChunk {          // a run of rays that is this wave's own: no atomics
    long next;
    __device__ __forceinline__ unsigned long long operator()(unsigned long long mask, int)
    {
        const long base = next;
        next += (long)__popcll(mask);
        return (unsigned long long)base;
    }
};
// One refill round: the lanes with `need` take consecutive rays from src in lane order.  False: no lane needs one, nothing was taken.  True:
// ray = this lane's index where need is set (the caller compares it with its ray count and sets the ray up: that part is each kernel's own).
template <class Src>
__device__ __forceinline__ bool march_take(Src& src, bool need, int lane, unsigned long long& ray)
{
    const unsigned long long mask = __ballot(need);
    if (!mask) return false;
    ray = src(mask, lane) + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
    return true;
}

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

// Density of a sample from the logit march_density left in sOut: sigma = exp(h0 - 1), 0 outside the model aabb.
__device__ __forceinline__ float march_sigma(bool inside_m, float h0) { return inside_m ? __expf(h0 - 1.f) : 0.f; }

// A renderer's step for one marched sample of a ray, in ray order: alpha = 1 - exp(-omega sigma dt); the sample SURVIVES iff T_all >= eps and
// (alpha_thre == 0 or alpha >= alpha_thre); T_all runs over all marched samples, T_s and the weight w = alpha T_s over the survivors only.
// omega: the overlap weight of render_pair.hip; the one-block renderers pass 1.f (1.f * sigma is sigma).
__device__ __forceinline__ bool march_composite(float sigma, float omega, float dt, float eps, float alpha_thre, float& T_all, float& T_s, float& w)
{
    const float sigma_eff = omega * sigma;
    const float alpha = 1.f - __expf(-sigma_eff * dt);
    const bool surv = T_all >= eps && (alpha_thre <= 0.f || alpha >= alpha_thre);
    T_all *= (1.f - alpha);
    if (surv) {
        w = alpha * T_s;
        T_s *= (1.f - alpha);
    }
    return surv;
}

// A survivor's input row of the colour net: fp16 SH4(d) in columns 0..15 and the constant 1 in column 31, around the 15 features march_density left.
__device__ __forceinline__ void march_color_row(char* sX, int lane, const uint32_t (&sh2)[8])
{
    uint32_t* xr = reinterpret_cast<uint32_t*>(sX + lane * NGP_XRS);
#pragma unroll
    for (int j = 0; j < 8; ++j) xr[j] = sh2[j];
    reinterpret_cast<_Float16*>(sX + lane * NGP_XRS)[31] = (_Float16)1.f;
}

// The colour net's first / last layer as this lane's MFMA operands (march_color's cw1f / cw3f).
__device__ __forceinline__ void march_load_color_w(f16x8_t (&cw1f)[4], f16x8_t (&cw3f)[2], const _Float16* cw1, const _Float16* cw3, int lane)
{
    const int fr = lane & 15, kg = lane >> 4;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) cw1f[cb] = *reinterpret_cast<const f16x8_t*>(cw1 + (cb * 16 + fr) * 32 + kg * 8);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) cw3f[kb] = *reinterpret_cast<const f16x8_t*>(cw3 + fr * 64 + kb * 32 + kg * 8);
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

// ---- the rules of registered blocks, shared by the two-block and the K-block renderer and by the density field of registered blocks

// Whether a block's own occupancy grid (binary uint8 [rdim], over the roi with low corner roi_lo and extents ext) covers the point x of the
// block's frame: inside the roi on all axes (u = (x - lo) / ext, 0 <= u <= 1) and the cell clamp(floor(u res), 0, res - 1) set.
__device__ __forceinline__ bool march_covered(const float* roi_lo, const float (&ext)[3], const int (&rdim)[3], const uint8_t* binary, const float (&x)[3])
{
    float u[3];
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) { u[k] = (x[k] - roi_lo[k]) / ext[k]; inside = inside && u[k] >= 0.f && u[k] <= 1.f; }
    if (!inside) return false;
    int ci[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ci[k] = min(max((int)floorf(u[k] * (float)rdim[k]), 0), rdim[k] - 1);
    return binary[((long)ci[0] * rdim[1] + ci[1]) * rdim[2] + ci[2]] != 0;
}

// A ray's cursor of block b, the ray given in the block's frame: act = the block is marched at all (the ray meets its scene aabb in a non-empty
// interval), n_lim = the lattice samples of the interval at most; a ray that misses keeps the empty interval [1, 0): nothing is marched and
// nothing is covered.  Each kernel stores the values where its cursor lives.
__device__ __forceinline__ bool march_cursor_ray(const MarchBlock& b, const float* origins, const float* dirs, long ray, float (&o)[3], float (&d)[3], float& tmin,
                                                 float& tmax, int& n_lim)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[k] = origins[ray * 3 + k]; d[k] = dirs[ray * 3 + k]; }
    const bool hit = render_ray_interval(o, d, b.scene, b.near, b.far, tmin, tmax);
    const bool act = hit && tmin < tmax;
    n_lim = 0;
    if (act) n_lim = (int)fminf(ceilf((tmax - tmin) / b.dt) + 1.f, (float)b.n_max);      // (n_max <= 1e8 + 2: the conversion cannot overflow)
    else { tmin = 1.f; tmax = 0.f; }
    return act;
}

// What a ray accumulates over the merged sample stream of its blocks; samples counts the lane's survivors over all its rays.
struct MarchAccum {
    float T_all, T_s, acc[3], opac, dep;
    unsigned long long samples;
};
__device__ __forceinline__ void march_accum_reset(MarchAccum& r)      // a new ray (samples runs on)
{
    r.T_all = 1.f; r.T_s = 1.f; r.acc[0] = r.acc[1] = r.acc[2] = 0.f; r.opac = 0.f; r.dep = 0.f;
}

// Density, compositing and colour of the lanes whose sample is of block b (have), at position x of that block's frame with direction dir, ray
// parameter tm and overlap weight omega: the per-sample arithmetic of ngp_render_kernel with sigma_eff = omega * sigma.  share(w) adds a
// survivor's weight to the block's own share of the ray, which is the caller's.  Skipped wave-uniformly when no lane has a sample of b.
template <class Share>
__device__ __forceinline__ void march_sample_phase(const MarchBlock& b, float eps, bool have, const float (&x)[3], const float (&dir)[3], float tm, float omega,
                                                   char* sX, char* sH, float* sOut, float* sO, MarchAccum& r, int lane, Share&& share)
{
    if (!__any(have)) return;
    bool surv = false;
    float w = 0.f;
    {
        NgpDensityW dw;
        ngp_load_density_w(dw, b.w1, b.w2, lane);
        const bool inside_m = march_density<true>(have, x, b.model, b.lv, b.table, dw, sX, sH, sOut, lane);
        if (have) {
            surv = march_composite(march_sigma(inside_m, sOut[lane]), omega, b.dt, eps, b.alpha_thre, r.T_all, r.T_s, w);
            if (surv) {
                uint32_t sh2[8];
                render_sh4_f16(dir, sh2);
                march_color_row(sX, lane, sh2);
            }
        }
    }
    if (__any(surv)) {
        f16x8_t cw1f[4], cw3f[2];
        march_load_color_w(cw1f, cw3f, b.cw1, b.cw3, lane);
        march_color(sX, sH, sH, sO, cw1f, b.cw2, cw3f, lane);
        if (surv) {
            const float4 pre = *reinterpret_cast<const float4*>(sO + lane * 4);
            const float pv[3] = {pre.x, pre.y, pre.z};
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) r.acc[ch] += w * march_sigmoid_f16(pv[ch]);
            r.opac += w;
            r.dep += w * tm;
            share(w);
            ++r.samples;
        }
    }
    wave_sync();
}

// The outputs every renderer of registered blocks writes for a finished ray: rgb over the background, opacity, depth.
__device__ __forceinline__ void march_write_ray(float* rgb, float* opacity, float* depth, const float (&bkgd)[3], long ray, const MarchAccum& r)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) rgb[ray * 3 + k] = r.acc[k] + bkgd[k] * (1.f - r.opac);
    opacity[ray] = r.opac;
    depth[ray] = r.dep;
}

// The tail of a persistent renderer.  march_count_samples: the survivors this wave composited, one atomic per wave.  march_report_overrun, called
// by lane 0 when the pass bound was reached with rays still queued or in flight: bit 63 of the ray counter (dreg_nerf_amd/render.py raises).
// (Two functions, the second under the caller's condition: as one function's argument the queue pointer was read unconditionally and held in
// SGPRs through the whole march.)
__device__ __forceinline__ void march_count_samples(unsigned long long samples, unsigned long long* n_samples, int lane)
{
    unsigned long long tot = samples;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off, 64);
    if (lane == 0 && tot) atomicAdd(n_samples, tot);
}
__device__ __forceinline__ void march_report_overrun(unsigned long long* queue) { atomicOr(queue, 1ull << 63); }
