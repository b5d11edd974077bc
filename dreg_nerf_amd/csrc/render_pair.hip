// Volume rendering of a REGISTERED PAIR of NeRF blocks as one scene, gfx950: a ray is marched through the source block S and the target
// block T at once and their samples are composited in depth order, in ONE persistent kernel that keeps no sample list (the two-block form of
// render.hip; rule: DESIGN.md §3e, CPU restatement: tests/render_pair_restatement.py).
//
// Frames.  The pose P = [R|t] maps the source frame to the target frame.  A ray (o, d) is given in the TARGET frame; block T marches it as
// it is, block S marches o_S = R^T (o - t), d_S = R^T d / |R^T d|, formed by the host in fp64 and rounded to fp32 (render.rays_to_block).
// The kernel receives the two origin / direction arrays and knows nothing of the pose; R is orthonormal to fp32 rounding, so both frames share
// the ray parameter t to ~1e-7 relative, far below any step.
//
// Per block b (its own scene aabb, near / far, dt_b, roi grid — §3b's march unchanged):
//   samples        t_mid = t_min_b + (n + 1/2) dt_b while t_mid < t_max_b, kept where b's own occupancy cell is set
// Merged stream    the two sample streams merged by t_mid; on a tie (t_S <= t_T) the source sample goes first
// Overlap weight   for a sample of block b at parameter t, the OTHER block b' covers it iff t in [t_min_b', t_max_b') and
//                  x_b' = o_b' + t d_b' lies inside the roi of b' in an occupied cell (floor + clamp lookup of march_advance, fine cells).
//                  Not covered: omega = 1.  Covered: with the camera centroids c_S, c_T of the blocks, each in its own frame,
//                  q = (|x_S - c_S|^2 + 1e-12) / (|x_T - c_T|^2 + 1e-12),  omega_S = 1 / (1 + q^(p/2)),  omega_T = 1 - omega_S   (p = power)
// Compositing      sigma_eff = omega sigma_b(x_b), alpha = 1 - exp(-sigma_eff dt_b), colour from the sample's own block with that block's
//                  direction; T_all, the survival test (T_all >= eps and (alpha_thre_b == 0 or alpha >= alpha_thre_b)), the weights over the
//                  survivors and the early stop (T_all < eps ends the ray) are §3b's, applied to the merged stream
// Outputs          rgb = sum w c + bkgd (1 - sum w), opacity = sum w, depth = sum w t_mid, weight_src = sum w over the SOURCE samples,
//                  n_samples = survivors.  A ray that misses both scene aabbs gets (bkgd, 0, 0, 0); one that meets one block only is that
//                  block's §3b render: with omega = 1 a sample's arithmetic is ngp_render_kernel's, operation for operation (1.f * sigma).
//
// One lane = one ray, one-wave workgroups, rays taken from a queue, the overrun report in bit 63 of the queue word — all as ngp_render_kernel.
// A lane keeps one cursor per block (origin, direction, interval, lattice index) and at most one pending sample per block.  Per pass every
// cursor without a pending sample advances (march_advance), a lane whose two cursors have each a pending sample or have ended takes the
// pending sample with the smaller t, and the wave runs, block by block, the density of the lanes on that block (march_density<true>) and
// the colour net of its survivors (march_color): S's density and colour, then T's.  (A block's colour follows its own density directly:
// march_density rewrites all 64 feature rows, so the features of S's samples would not outlive T's density phase.)  Each phase is skipped
// wave-uniformly when no lane needs it.
// Registers: two sets of MFMA operands do not fit beside the march state at two waves per SIMD, so a block's operands (14 KB per block,
// L2-resident) are loaded at the head of its phase and SH4(d) is formed per surviving sample instead of being held per ray — the same
// function of the same direction, hence the same bits.  The two phases are ONE loop body over the block index (not unrolled) that reads the
// block's arguments from the kernel-argument segment: written out per block, both blocks' pointers and aabbs were hoisted into SGPRs and
// spilled, and the kernel reserved scratch.  As built: 225 VGPRs, no scratch, 23.8 KB of LDS (six workgroups per CU), DESIGN.md §3e.
// A ray's result depends on nothing but its own samples: output is bit-identical between runs and launch widths.
#include "march.h"
#include "../../include/dreg_nerf.h"   // signature check of the entry point defined here

struct PairBlock : MarchBlock {
    const float* origins;       // [N,3] in this block's frame
    const float* dirs;          // [N,3] unit viewing directions in this block's frame
    float center[3];            // centroid of the block's cameras, in the block's frame
};

struct PairArgs {
    PairBlock b[2];             // 0 = source, 1 = target
    long n_rays;
    float half_power, eps;
    float bkgd[3];
    long pass_bound;            // n_rays * (n_max_S + n_max_T + 2) + 64: every pass takes a ray, a sample or a lattice step
    float *rgb, *opacity, *depth, *weight_src;
    unsigned long long* n_samples;
    unsigned long long* queue;
};

DREG_KNOB(int, g_render_pair_waves, 2048);     // tuning (include/dreg_nerf_probe.h): one-wave workgroups of the launch

// One block's march state of a lane's ray.  act: the cursor can still advance; pend: a sample at t_mid = tp waits to be composited.
// A ray that misses the block keeps the empty interval [1, 0): nothing is marched and nothing is covered.
struct PairCursor {
    float o[3], d[3], tmin, tmax, tp;
    int n, n_lim;
    bool act, pend;
};

__device__ __forceinline__ void pair_take_ray(const PairBlock& b, PairCursor& c, long ray)
{
    c.act = march_cursor_ray(b, b.origins, b.dirs, ray, c.o, c.d, c.tmin, c.tmax, c.n_lim);
    c.pend = false; c.n = 0; c.tp = 0.f;
}

// the cursor's next occupied lattice sample, if it has none pending (ngp_render_kernel's advance step)
__device__ __forceinline__ void pair_advance(const MarchGrid& g, const PairBlock& b, PairCursor& c, bool live)
{
    const bool wanted = live && c.act && !c.pend;
    bool adv = wanted;
    if (adv && c.n >= c.n_lim) adv = false;                       // (never taken: t_mid >= t_max ends a cursor first; the argument-derived bound)
    float x[3] = {0.f, 0.f, 0.f}, tm = 0.f;
    const bool got = march_advance(g, c.o, c.d, c.tmin, c.tmax, b.dt, c.n, adv, x, &tm, 4096);
    if (got) { c.pend = true; c.tp = tm; }
    if (wanted && !adv) c.act = false;                            // left [t_min, t_max)
}

// whether the block of cursor c covers the parameter t of its ray, x = o + t d: inside its interval, inside its roi, in an occupied fine cell
__device__ __forceinline__ bool pair_covered(const MarchGrid& g, const PairCursor& c, float t, const float (&x)[3])
{
    return t >= c.tmin && t < c.tmax && march_covered(g.roi, g.roi_ext, g.rdim, g.binary, x);
}

struct PairAccum : MarchAccum {
    float wsrc;                 // the source block's share: sum w over its samples
};

__device__ __forceinline__ void pair_write(const PairArgs& a, long ray, const PairAccum& r)
{
    march_write_ray(a.rgb, a.opacity, a.depth, a.bkgd, ray, r);
    a.weight_src[ray] = r.wsrc;
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void ngp_render_pair_kernel(PairArgs a)
{
    __shared__ __attribute__((aligned(16))) char sX[64 * NGP_XRS];
    __shared__ __attribute__((aligned(16))) char sH[64 * NGP_HRS];
    __shared__ float sOut[64];
    __shared__ __attribute__((aligned(16))) float sO[64 * 4];
    __shared__ uint32_t sCoarse[2][1024];
    const int lane = threadIdx.x;
    march_load_coarse(sCoarse[0], a.b[0], lane);
    march_load_coarse(sCoarse[1], a.b[1], lane);
    __syncthreads();
    MarchGrid g0, g1;
    march_grid(g0, a.b[0], sCoarse[0]);
    march_grid(g1, a.b[1], sCoarse[1]);
    MarchQueue queue = {a.queue};

    // per-lane ray state
    bool live = false, exhausted = false;
    long ray = 0;
    PairCursor c0, c1;
#pragma unroll
    for (int k = 0; k < 3; ++k) { c0.o[k] = c1.o[k] = 0.f; c0.d[k] = c1.d[k] = 0.f; }
    c0.tmin = c1.tmin = 1.f; c0.tmax = c1.tmax = 0.f; c0.tp = c1.tp = 0.f;
    c0.n = c1.n = 0; c0.n_lim = c1.n_lim = 0; c0.act = c1.act = false; c0.pend = c1.pend = false;
    PairAccum r;
    march_accum_reset(r);
    r.wsrc = 0.f; r.samples = 0;

    bool finished = false;
    for (long it = 0; it < a.pass_bound; ++it) {
        // ---- refill: lanes without a ray take the next ones from the queue; rays that miss both aabbs are written at once
        for (int tries = 0; tries < 1024; ++tries) {
            const bool need = !live && !exhausted;
            unsigned long long q = 0;
            if (!march_take(queue, need, lane, q)) break;
            if (need) {
                if (q >= (unsigned long long)a.n_rays) exhausted = true;
                else {
                    ray = (long)q;
                    pair_take_ray(a.b[0], c0, ray);
                    pair_take_ray(a.b[1], c1, ray);
                    march_accum_reset(r);
                    r.wsrc = 0.f;
                    if (c0.act || c1.act) live = true;
                    else pair_write(a, ray, r);
                }
            }
        }
        if (!__any(live)) {
            if (__all(exhausted)) { finished = true; break; }        // the queue is empty and nothing is in flight
            continue;                                                // (a long run of missed rays used up this pass's refill rounds)
        }
        // ---- every cursor without a pending sample advances to its next lattice sample inside an occupied cell of its block
        pair_advance(g0, a.b[0], c0, live);
        pair_advance(g1, a.b[1], c1, live);
        if (live && !c0.act && !c1.act && !c0.pend && !c1.pend) { live = false; pair_write(a, ray, r); }     // both blocks left behind
        // ---- a lane whose two cursors have each a pending sample or have ended takes the nearer one (the source's on a tie)
        const bool ready = live && (c0.pend || !c0.act) && (c1.pend || !c1.act);
        if (!__any(ready)) continue;
        const bool pick_s = c0.pend && (!c1.pend || c0.tp <= c1.tp);
        const bool have_s = ready && pick_s, have_t = ready && !pick_s;
        const float tm = pick_s ? c0.tp : c1.tp;
        float xs[3], xt[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { xs[k] = c0.o[k] + tm * c0.d[k]; xt[k] = c1.o[k] + tm * c1.d[k]; }
        // ---- overlap weight: where the other block covers the sample too, the blocks share it by inverse distance to their cameras
        float omega = 1.f;
        if (ready) {
            const bool covered = pick_s ? pair_covered(g1, c1, tm, xt) : pair_covered(g0, c0, tm, xs);
            if (covered) {
                float ds = 0.f, dt2 = 0.f;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float es = xs[k] - a.b[0].center[k], et = xt[k] - a.b[1].center[k];
                    ds += es * es; dt2 += et * et;
                }
                const float q = (ds + 1e-12f) / (dt2 + 1e-12f);
                const float ws = 1.f / (1.f + __expf(a.half_power * __logf(q)));                 // 1 / (1 + q^(p/2))
                omega = pick_s ? ws : 1.f - ws;
            }
            if (pick_s) { c0.pend = false; ++c0.n; } else { c1.pend = false; ++c1.n; }
        }
        // ---- the sample's own position and direction; one body serves both blocks (the block's arguments are read per phase, not held)
        float xp[3], dp[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { xp[k] = pick_s ? xs[k] : xt[k]; dp[k] = pick_s ? c0.d[k] : c1.d[k]; }
#pragma unroll 1
        for (int q = 0; q < 2; ++q)
            march_sample_phase(a.b[q], a.eps, q == 0 ? have_s : have_t, xp, dp, tm, omega, sX, sH, sOut, sO, r, lane, [&](float w) { if (q == 0) r.wsrc += w; });
        if (ready && r.T_all < a.eps) { live = false; pair_write(a, ray, r); }           // transmittance below early_stop_eps: the ray ends
    }
    march_count_samples(r.samples, a.n_samples, lane);
    if (!finished && lane == 0) march_report_overrun(a.queue);
}

// One block's arguments as dreg_ngp_render takes them, plus the camera centroid.
struct PairBlockHost {
    const float *origins, *viewdirs;
    const uint8_t* binary;
    int rx, ry, rz;
    const uint32_t* coarse_bits;
    const void *table, *w1, *w2, *cw1, *cw2, *cw3;
    const uint32_t *offset, *size, *res;
    const float* scale;
    const uint32_t* hashed;
    const float *roi_aabb, *scene_aabb, *model_aabb;
    float near_plane, far_plane, render_step_size, alpha_thre;
    const float* center;
};

static int pair_fill_block(PairBlock& b, const PairBlockHost& h)
{
    if (!h.origins || !h.viewdirs || !h.center) return DREG_EINVAL;
    b.origins = h.origins; b.dirs = h.viewdirs;
    for (int k = 0; k < 3; ++k) b.center[k] = h.center[k];
    return march_fill_block(b, h.binary, h.rx, h.ry, h.rz, h.coarse_bits, h.table, h.w1, h.w2, true, h.cw1, h.cw2, h.cw3, h.offset, h.size, h.res, h.scale,
                            h.hashed, h.roi_aabb, h.scene_aabb, h.model_aabb, h.near_plane, h.far_plane, h.render_step_size, h.alpha_thre, true);
}

static int render_pair_launch(const PairBlockHost& src, const PairBlockHost& tgt, long n_rays, float power, float early_stop_eps, const float* bkgd,
                              float* rgb, float* opacity, float* depth, float* weight_src, unsigned long long* n_samples, void* queue, void* stream)
{
    if (n_rays < 0 || !(power >= 0.f) || !(power <= 1e4f)) return DREG_EINVAL;
    if (n_rays == 0) return DREG_OK;
    if (!bkgd || !rgb || !opacity || !depth || !weight_src || !n_samples || !queue) return DREG_EINVAL;
    PairArgs a;
    if (pair_fill_block(a.b[0], src) != DREG_OK || pair_fill_block(a.b[1], tgt) != DREG_OK) return DREG_EINVAL;
    a.n_rays = n_rays; a.half_power = 0.5f * power; a.eps = early_stop_eps;
    for (int k = 0; k < 3; ++k) a.bkgd[k] = bkgd[k];
    a.pass_bound = march_pass_bound(n_rays, (double)a.b[0].n_max + (double)a.b[1].n_max + 2.0);
    a.rgb = rgb; a.opacity = opacity; a.depth = depth; a.weight_src = weight_src; a.n_samples = n_samples; a.queue = (unsigned long long*)queue;
    long waves = (n_rays + 63) / 64;
    if (waves > g_render_pair_waves) waves = g_render_pair_waves;
    hipLaunchKernelGGL(ngp_render_pair_kernel, dim3((unsigned)waves), dim3(64), 0, (hipStream_t)stream, a);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

extern "C" {

// Render n_rays rays through the source block (src_*) and the target block (tgt_*) as one scene.  Per block the arguments are dreg_ngp_render's
// (caller-owned device buffers; level arrays and aabbs are HOST pointers) with the rays in that block's frame, plus center: the centroid of the
// block's cameras in its frame, 3 floats in HOST memory.  Shared: power (p of the overlap weight), early_stop_eps, bkgd (host), the outputs
// rgb fp32 [N,3], opacity / depth / weight_src fp32 [N], n_samples: one u64 and queue: 8 bytes, both zeroed by the caller on `stream`.
int dreg_ngp_render_pair(long n_rays,
                         const float* src_origins, const float* src_viewdirs, const uint8_t* src_binary, int src_rx, int src_ry, int src_rz,
                         const uint32_t* src_coarse_bits, const void* src_table, const void* src_w1, const void* src_w2,
                         const void* src_cw1, const void* src_cw2, const void* src_cw3,
                         const uint32_t* src_offset, const uint32_t* src_size, const uint32_t* src_res, const float* src_scale, const uint32_t* src_hashed,
                         const float* src_roi_aabb, const float* src_scene_aabb, const float* src_model_aabb,
                         float src_near_plane, float src_far_plane, float src_render_step_size, float src_alpha_thre, const float* src_center,
                         const float* tgt_origins, const float* tgt_viewdirs, const uint8_t* tgt_binary, int tgt_rx, int tgt_ry, int tgt_rz,
                         const uint32_t* tgt_coarse_bits, const void* tgt_table, const void* tgt_w1, const void* tgt_w2,
                         const void* tgt_cw1, const void* tgt_cw2, const void* tgt_cw3,
                         const uint32_t* tgt_offset, const uint32_t* tgt_size, const uint32_t* tgt_res, const float* tgt_scale, const uint32_t* tgt_hashed,
                         const float* tgt_roi_aabb, const float* tgt_scene_aabb, const float* tgt_model_aabb,
                         float tgt_near_plane, float tgt_far_plane, float tgt_render_step_size, float tgt_alpha_thre, const float* tgt_center,
                         float power, float early_stop_eps, const float* bkgd,
                         float* rgb, float* opacity, float* depth, float* weight_src, unsigned long long* n_samples, void* queue, void* stream)
{
    const PairBlockHost src = {src_origins, src_viewdirs, src_binary, src_rx, src_ry, src_rz, src_coarse_bits, src_table, src_w1, src_w2,
                               src_cw1, src_cw2, src_cw3, src_offset, src_size, src_res, src_scale, src_hashed, src_roi_aabb, src_scene_aabb,
                               src_model_aabb, src_near_plane, src_far_plane, src_render_step_size, src_alpha_thre, src_center};
    const PairBlockHost tgt = {tgt_origins, tgt_viewdirs, tgt_binary, tgt_rx, tgt_ry, tgt_rz, tgt_coarse_bits, tgt_table, tgt_w1, tgt_w2,
                               tgt_cw1, tgt_cw2, tgt_cw3, tgt_offset, tgt_size, tgt_res, tgt_scale, tgt_hashed, tgt_roi_aabb, tgt_scene_aabb,
                               tgt_model_aabb, tgt_near_plane, tgt_far_plane, tgt_render_step_size, tgt_alpha_thre, tgt_center};
    return render_pair_launch(src, tgt, n_rays, power, early_stop_eps, bkgd, rgb, opacity, depth, weight_src, n_samples, queue, stream);
}

#ifdef DREG_PROBE
void dreg_render_pair_set_waves(int n) { g_render_pair_waves = n > 0 ? n : 2048; }
#endif

}  // extern "C"
