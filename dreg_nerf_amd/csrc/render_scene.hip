// Volume rendering of a REGISTERED SCENE of K NeRF blocks (1 <= K <= DREG_SCENE_MAX_BLOCKS = 4) as one scene, gfx950: a ray is marched through
// all K blocks at once and their samples are composited in depth order, in ONE persistent kernel that keeps no sample list (the K-block form of
// render_pair.hip; rule: DESIGN.md §3j, CPU restatement: tests/render_scene_restatement.py).
//
// Frames.  Block b has a pose G_b that maps its frame to the frame the rays are given in; the host brings the rays into every block's frame
// (render.rays_to_block, fp64, rounded to fp32) and the kernel receives K origin / direction arrays and knows nothing of the poses.
//
// Per block b    §3b's march on the block's own lattice: t_mid = t_min_b + (n + 1/2) dt_b while t_mid < t_max_b, kept where b's own cell is set
// Merged stream  the K sample streams merged by t_mid; on a tie the LOWEST block index goes first (K = 2: render_pair.hip's "source first")
// Coverage       another block b' covers a sample at parameter t iff t in [t_min_b', t_max_b') and x_b' = o_b' + t d_b' lies inside the roi of
//                b' in an occupied fine cell (floor + clamp lookup) — pair_covered's rule
// Overlap weight C = the other blocks that cover the sample, delta_b = |x_b - c_b|^2 + 1e-12 with the camera centroid c_b of block b:
//                |C| = 0: omega = 1
//                |C| = 1: the pair's rule, operation for operation: with lo / hi the lower / higher block index of the two,
//                         q = delta_lo / delta_hi, omega_lo = 1 / (1 + expf(p/2 logf(q))), omega_hi = 1 - omega_lo
//                |C| >= 2: omega_b = 1 / (1 + sum over b' in C, ascending, of expf(p/2 logf(delta_b / delta_b')))
// Compositing    march_composite with sigma_eff = omega sigma on the merged stream: T_all, survival, weights over the survivors, early stop
// Outputs        rgb, opacity, depth as render_pair.hip; weight_block [N,K] = sum w over the samples of each block; n_samples = survivors.
// With K = 2 a sample's arithmetic is ngp_render_pair_kernel's, and with all grids empty but one ngp_render_kernel's: bit for bit
// (tests/test_hip_render_scene.py).
//
// One lane = one ray, one-wave workgroups, rays from a MarchQueue, the overrun report in bit 63 of the queue word — all as ngp_render_pair_kernel.
// A lane keeps one cursor per block (origin, direction, interval, lattice index, pending sample).  The pair kernel holds its two 13-dword cursors
// in registers at 225 VGPRs; four do not fit at two waves per SIMD, and a per-lane array indexed by a run-time block index would go to scratch.
// The cursors therefore live in LDS, lane-major (dword f of block b of lane l at (b * 13 + f) * 64 + l: a wave's access is conflict-free and a
// lane touches only its own column, so no barrier is needed); a cursor is read into registers for the block loop body that works on it, and the
// picked block's cursor is read with the LANE's block index.  The camera centroids sit in LDS too, for the same lane-indexed read.
// Every loop over the block index is ONE non-unrolled body that reads the block from the kernel-argument segment (render_pair.hip's header says
// what happened when that body was written out per block).  Resources as built: DESIGN.md §3j.
#include "march.h"
#include "../../include/dreg_nerf.h"   // dreg_scene_block, DREG_SCENE_MAX_BLOCKS and the signature check of the entry point defined here

#define SCENE_MAXB DREG_SCENE_MAX_BLOCKS

struct SceneBlock : MarchBlock {
    const float* origins;       // [N,3] in this block's frame
    const float* dirs;          // [N,3] unit viewing directions in this block's frame
    float center[3];            // centroid of the block's cameras, in the block's frame
};

struct SceneArgs {
    SceneBlock b[SCENE_MAXB];   // the first K are filled, the rest zero
    int K;
    long n_rays;
    float half_power, eps;
    float bkgd[3];
    long pass_bound;            // n_rays * (sum_b n_max_b + 2) + 64: every pass takes a ray, a sample or a lattice step
    float *rgb, *opacity, *depth, *weight_block;
    unsigned long long* n_samples;
    unsigned long long* queue;
};
static_assert(sizeof(SceneArgs) <= 4096, "the blocks are read from the kernel-argument segment");

DREG_KNOB(int, g_render_scene_waves, 2048);    // tuning (include/dreg_nerf_probe.h): one-wave workgroups of the launch

// A cursor = one block's march state of a lane's ray, 13 dwords in LDS.  act: the cursor can still advance; pend: a sample at t_mid = tp waits
// to be composited.  A ray that misses the block keeps the empty interval [1, 0): nothing is marched and nothing is covered.
enum { CUR_O = 0, CUR_D = 3, CUR_TMIN = 6, CUR_TMAX = 7, CUR_TP = 8, CUR_N = 9, CUR_NLIM = 10, CUR_ACT = 11, CUR_PEND = 12, CUR_DW = 13 };
#define CURF(b, f) sCur[((b) * CUR_DW + (f)) * 64 + lane]
#define CURI(b, f) reinterpret_cast<int*>(sCur)[((b) * CUR_DW + (f)) * 64 + lane]

// the ray's cursor of block b into its LDS column; returns whether the block is marched at all
__device__ __forceinline__ bool scene_take_ray(const SceneBlock& b, float* sCur, int bi, long ray, int lane)
{
    float o[3], d[3], tmin, tmax;
    int n_lim;
    const bool act = march_cursor_ray(b, b.origins, b.dirs, ray, o, d, tmin, tmax, n_lim);
#pragma unroll
    for (int k = 0; k < 3; ++k) { CURF(bi, CUR_O + k) = o[k]; CURF(bi, CUR_D + k) = d[k]; }
    CURF(bi, CUR_TMIN) = tmin; CURF(bi, CUR_TMAX) = tmax; CURF(bi, CUR_TP) = 0.f;
    CURI(bi, CUR_N) = 0; CURI(bi, CUR_NLIM) = n_lim; CURI(bi, CUR_ACT) = act ? 1 : 0; CURI(bi, CUR_PEND) = 0;
    return act;
}

struct SceneAccum : MarchAccum {
    float wb[SCENE_MAXB];       // the blocks' shares: sum w over the samples of each
};

__device__ __forceinline__ void scene_reset(SceneAccum& r)
{
    march_accum_reset(r);
#pragma unroll
    for (int j = 0; j < SCENE_MAXB; ++j) r.wb[j] = 0.f;
}

__device__ __forceinline__ void scene_write(const SceneArgs& a, long ray, const SceneAccum& r)
{
    march_write_ray(a.rgb, a.opacity, a.depth, a.bkgd, ray, r);
#pragma unroll
    for (int j = 0; j < SCENE_MAXB; ++j)
        if (j < a.K) a.weight_block[ray * a.K + j] = r.wb[j];
}

// (waves per SIMD 1..2: the registers are held to the pair kernel's budget of two waves, the 44.3 KB of LDS admit three workgroups per CU)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void ngp_render_scene_kernel(SceneArgs a)
{
    __shared__ __attribute__((aligned(16))) char sX[64 * NGP_XRS];
    __shared__ __attribute__((aligned(16))) char sH[64 * NGP_HRS];
    __shared__ float sOut[64];
    __shared__ __attribute__((aligned(16))) float sO[64 * 4];
    __shared__ uint32_t sCoarse[SCENE_MAXB][1024];
    __shared__ float sCur[SCENE_MAXB * CUR_DW * 64];
    __shared__ float sCenter[SCENE_MAXB * 3];
    const int lane = threadIdx.x;
    const int K = a.K;
#pragma unroll 1
    for (int b = 0; b < K; ++b) {
        march_load_coarse(sCoarse[b], a.b[b], lane);
        if (lane < 3) sCenter[b * 3 + lane] = lane == 0 ? a.b[b].center[0] : lane == 1 ? a.b[b].center[1] : a.b[b].center[2];
    }
    for (int i = lane; i < SCENE_MAXB * CUR_DW * 64; i += 64) sCur[i] = 0.f;      // (every cursor starts ended, with nothing pending)
    __syncthreads();
    MarchQueue queue = {a.queue};

    // per-lane ray state
    bool live = false, exhausted = false;
    long ray = 0;
    SceneAccum r;
    scene_reset(r);
    r.samples = 0;

    bool finished = false;
    for (long it = 0; it < a.pass_bound; ++it) {
        // ---- refill: lanes without a ray take the next ones from the queue; rays that miss every aabb are written at once
        for (int tries = 0; tries < 1024; ++tries) {
            const bool need = !live && !exhausted;
            unsigned long long q = 0;
            if (!march_take(queue, need, lane, q)) break;
            if (need) {
                if (q >= (unsigned long long)a.n_rays) exhausted = true;
                else {
                    ray = (long)q;
                    bool any = false;
#pragma unroll 1
                    for (int b = 0; b < K; ++b) any = scene_take_ray(a.b[b], sCur, b, ray, lane) || any;
                    scene_reset(r);
                    if (any) live = true;
                    else scene_write(a, ray, r);
                }
            }
        }
        if (!__any(live)) {
            if (__all(exhausted)) { finished = true; break; }        // the queue is empty and nothing is in flight
            continue;                                                // (a long run of missed rays used up this pass's refill rounds)
        }
        // ---- every cursor without a pending sample advances to its next lattice sample inside an occupied cell of its block; the lane's
        //      nearest pending sample is found on the way (strictly nearer replaces: the lowest block index wins a tie)
        bool all_ready = true, any_alive = false;
        int pick = 0;
        bool picked = false;
        float tm = 0.f;
#pragma unroll 1
        for (int b = 0; b < K; ++b) {
            bool act = CURI(b, CUR_ACT) != 0, pend = CURI(b, CUR_PEND) != 0;
            float tp = CURF(b, CUR_TP);
            const bool wanted = live && act && !pend;
            if (__any(wanted)) {
                float o[3], d[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) { o[k] = CURF(b, CUR_O + k); d[k] = CURF(b, CUR_D + k); }
                const float tmin = CURF(b, CUR_TMIN), tmax = CURF(b, CUR_TMAX);
                int n = CURI(b, CUR_N);
                MarchGrid g;
                march_grid(g, a.b[b], sCoarse[b]);
                bool adv = wanted;
                if (adv && n >= CURI(b, CUR_NLIM)) adv = false;           // (never taken: t_mid >= t_max ends a cursor first; the argument-derived bound)
                float x[3] = {0.f, 0.f, 0.f}, t_new = 0.f;
                const bool got = march_advance(g, o, d, tmin, tmax, a.b[b].dt, n, adv, x, &t_new, 4096);
                if (got) { pend = true; tp = t_new; CURF(b, CUR_TP) = t_new; CURI(b, CUR_PEND) = 1; }
                if (wanted && !adv) { act = false; CURI(b, CUR_ACT) = 0; }    // left [t_min, t_max)
                if (wanted) CURI(b, CUR_N) = n;
            }
            all_ready = all_ready && (pend || !act);
            any_alive = any_alive || act || pend;
            if (pend && (!picked || tp < tm)) { picked = true; pick = b; tm = tp; }
        }
        if (live && !any_alive) { live = false; scene_write(a, ray, r); }      // every block left behind
        // ---- a lane whose cursors have each a pending sample or have ended takes the nearest one
        const bool ready = live && all_ready;
        if (!__any(ready)) continue;
        if (!ready) { pick = 0; tm = 0.f; }
        // ---- the sample's own position and direction, from the picked block's cursor
        float xp[3], dp[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { dp[k] = CURF(pick, CUR_D + k); xp[k] = CURF(pick, CUR_O + k) + tm * dp[k]; }
        // ---- overlap weight: the blocks that cover the sample share it by inverse distance to their cameras
        float omega = 1.f;
        if (ready) {
            float d_own = 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) { const float e = xp[k] - sCenter[pick * 3 + k]; d_own += e * e; }
            d_own += 1e-12f;
            int cnt = 0;
            bool first_lower = false;
            float d_first = 1.f, sum = 0.f;
#pragma unroll 1
            for (int b = 0; b < K; ++b) {
                if (b == pick) continue;
                if (!(tm >= CURF(b, CUR_TMIN) && tm < CURF(b, CUR_TMAX))) continue;
                float xo[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) xo[k] = CURF(b, CUR_O + k) + tm * CURF(b, CUR_D + k);
                MarchGrid g;
                march_grid(g, a.b[b], sCoarse[b]);
                if (!march_covered(g.roi, g.roi_ext, g.rdim, g.binary, xo)) continue;
                float d_oth = 0.f;
#pragma unroll
                for (int k = 0; k < 3; ++k) { const float e = xo[k] - a.b[b].center[k]; d_oth += e * e; }
                d_oth += 1e-12f;
                if (cnt == 0) { first_lower = b < pick; d_first = d_oth; }
                sum += __expf(a.half_power * __logf(d_own / d_oth));
                ++cnt;
            }
            if (cnt == 1 && first_lower) omega = 1.f - 1.f / (1.f + __expf(a.half_power * __logf(d_first / d_own)));     // the pair's omega_hi = 1 - omega_lo
            else if (cnt >= 1) omega = 1.f / (1.f + sum);
            CURI(pick, CUR_PEND) = 0;
            CURI(pick, CUR_N) = CURI(pick, CUR_N) + 1;
        }
        // ---- one body serves all blocks (the block's arguments are read per phase, not held)
#pragma unroll 1
        for (int q = 0; q < K; ++q)
            march_sample_phase(a.b[q], a.eps, ready && pick == q, xp, dp, tm, omega, sX, sH, sOut, sO, r, lane, [&](float w) {
#pragma unroll
                for (int j = 0; j < SCENE_MAXB; ++j) r.wb[j] += (j == q) ? w : 0.f;      // (the other shares take + 0.f: the accumulators are not indexed at run time)
            });
        if (ready && r.T_all < a.eps) { live = false; scene_write(a, ray, r); }          // transmittance below early_stop_eps: the ray ends
    }
    march_count_samples(r.samples, a.n_samples, lane);
    if (!finished && lane == 0) march_report_overrun(a.queue);
}

static int scene_fill_block(SceneBlock& b, const dreg_scene_block& h)
{
    if (!h.origins || !h.viewdirs || !h.center) return DREG_EINVAL;
    b.origins = h.origins; b.dirs = h.viewdirs;
    for (int k = 0; k < 3; ++k) b.center[k] = h.center[k];
    return march_fill_block(b, h.binary, h.rx, h.ry, h.rz, h.coarse_bits, h.table, h.w1, h.w2, true, h.cw1, h.cw2, h.cw3, h.offset, h.size, h.res, h.scale,
                            h.hashed, h.roi_aabb, h.scene_aabb, h.model_aabb, h.near_plane, h.far_plane, h.render_step_size, h.alpha_thre, true);
}

extern "C" {

// Render n_rays rays through the n_blocks blocks of `blocks` (HOST array) as one scene; see include/dreg_nerf.h.
int dreg_ngp_render_scene(long n_rays, int n_blocks, const dreg_scene_block* blocks, float power, float early_stop_eps, const float* bkgd,
                          float* rgb, float* opacity, float* depth, float* weight_block, unsigned long long* n_samples, void* queue, void* stream)
{
    if (n_blocks < 1 || n_blocks > SCENE_MAXB || !blocks) return DREG_EINVAL;
    if (n_rays < 0 || !(power >= 0.f) || !(power <= 1e4f)) return DREG_EINVAL;
    if (n_rays == 0) return DREG_OK;
    if (!bkgd || !rgb || !opacity || !depth || !weight_block || !n_samples || !queue) return DREG_EINVAL;
    SceneArgs a;
    __builtin_memset(&a, 0, sizeof(a));
    double steps = 2.0;
    for (int b = 0; b < n_blocks; ++b) {
        if (scene_fill_block(a.b[b], blocks[b]) != DREG_OK) return DREG_EINVAL;
        steps += (double)a.b[b].n_max;
    }
    a.K = n_blocks; a.n_rays = n_rays; a.half_power = 0.5f * power; a.eps = early_stop_eps;
    for (int k = 0; k < 3; ++k) a.bkgd[k] = bkgd[k];
    a.pass_bound = march_pass_bound(n_rays, steps);
    a.rgb = rgb; a.opacity = opacity; a.depth = depth; a.weight_block = weight_block; a.n_samples = n_samples; a.queue = (unsigned long long*)queue;
    long waves = (n_rays + 63) / 64;
    if (waves > g_render_scene_waves) waves = g_render_scene_waves;
    hipLaunchKernelGGL(ngp_render_scene_kernel, dim3((unsigned)waves), dim3(64), 0, (hipStream_t)stream, a);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

#ifdef DREG_PROBE
void dreg_render_scene_set_waves(int n) { g_render_scene_waves = n > 0 ? n : 2048; }
#endif

}  // extern "C"
