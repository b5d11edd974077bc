// Volume rendering of one NeRF block (Instant-NGP field + occupancy grid), gfx950: the reference's render_image
// (conerf/utils/utils.py:44-141) = nerfacc 0.3.5 ray_marching(sigma_fn, early_stop_eps = 1e-4, alpha_thre, stratified = False) followed by
// rendering(rgb_sigma_fn, render_bkgd), in ONE persistent kernel that keeps no sample list.  nerfacc is absent from the reference tree: parity
// is unpinned, the rule below is the specification (DESIGN.md "Volume renderer"; CPU restatement: tests/render_restatement.py).
//
// For a ray with origin o and unit direction d (the reference marches along viewdirs):
//   t_min, t_max   slab test against the scene aabb (t_min clamped at 0), then t_min = max(t_min, near), t_max = min(t_max, far);
//                  a ray that misses the aabb has no samples
//   samples        t_mid = t_min + (n + 1/2) dt while t_mid < t_max, kept only where the occupancy cell (over the roi aabb, floor + clamp;
//                  outside the roi = unoccupied) is set
//   alpha          1 - exp(-sigma(o + t_mid d) dt)
//   T_all          exclusive product of (1 - alpha) over ALL marched samples; a sample SURVIVES iff T_all >= early_stop_eps and
//                  (alpha_thre == 0 or alpha >= alpha_thre); the ray ends once T_all < early_stop_eps
//   weights        over the survivors only: w_k = alpha_k prod_{j<k, j survives} (1 - alpha_j)   (rendering() of the pruned list)
//   outputs        rgb = sum w c + bkgd (1 - sum w), opacity = sum w, depth = sum w t_mid (not normalised), n_samples = survivors
//
// One lane = one ray.  A lane whose ray has ended takes the next one from a queue (one atomic per wave and refill, as vis_march_queue).  Per
// pass every live lane advances to its next occupied lattice sample (march.h), the wave evaluates the 64 densities together on fp16 MFMA,
// each lane composites its own sample in ray order, and the colour net (SH4(d) | 15 features | 1 -> 64 -> 64 -> 3, sigmoid: the arithmetic of
// ngp_rgb_kernel with per-point directions) runs only when some lane's sample survived — the rows of surviving lanes are the live ones.
// SH4(d) is formed once per ray.  A ray's result depends on nothing but its own samples: output is bit-identical between runs and launch widths.
#include "march.h"
#include "../../include/dreg_nerf.h"   // signature check of the entry point defined here

struct RenderArgs : MarchBlock {       // the block (march.h; every ray's ceil((t_max - t_min) / dt) + 1 is below its n_max), then the launch's own
    const float* origins;       // [N,3]
    const float* dirs;          // [N,3] unit viewing directions
    const float* jitter;        // [N] per-ray u in [0,1) of stratified marching (dreg_ngp_render_train); null = 0 (dreg_ngp_render)
    long n_rays;
    float eps;
    float bkgd[3];
    long pass_bound;            // passes of the march loop per wave: n_rays * (n_max + 2) + 64 (march_pass_bound)
    float *rgb, *opacity, *depth;
    unsigned long long* n_samples;
    unsigned long long* queue;
};

DREG_KNOB(int, g_render_waves, 2048);     // tuning (include/dreg_nerf_probe.h): one-wave workgroups of the launch (256 CUs x 8: 19.7 KB of LDS each)

__device__ __forceinline__ void render_write(const RenderArgs& a, long ray, const float (&acc)[3], float opac, float dep)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) a.rgb[ray * 3 + k] = acc[k] + a.bkgd[k] * (1.f - opac);
    a.opacity[ray] = opac;
    a.depth[ray] = dep;
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void ngp_render_kernel(RenderArgs a)
{
    __shared__ __attribute__((aligned(16))) char sX[64 * NGP_XRS];
    __shared__ __attribute__((aligned(16))) char sH[64 * NGP_HRS];
    __shared__ float sOut[64];
    __shared__ __attribute__((aligned(16))) float sO[64 * 4];
    __shared__ uint32_t sCoarse[1024];
    const int lane = threadIdx.x;
    march_load_coarse(sCoarse, a, lane);
    __syncthreads();
    MarchGrid g;
    march_grid(g, a, sCoarse);
    NgpDensityW dw;
    ngp_load_density_w(dw, a.w1, a.w2, lane);
    f16x8_t cw1f[4], cw3f[2];
    march_load_color_w(cw1f, cw3f, a.cw1, a.cw3, lane);
    MarchQueue queue = {a.queue};

    // per-lane ray state
    bool active = false, exhausted = false;
    long ray = 0;
    int n = 0, n_lim = 0;
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f}, tmin = 0.f, tmax = 0.f;
    float T_all = 1.f, T_s = 1.f, acc[3] = {0.f, 0.f, 0.f}, opac = 0.f, dep = 0.f;
    uint32_t sh2[8];            // fp16 SH4(d), two per word
    unsigned long long my_samples = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) sh2[j] = 0u;

    bool finished = false;
    for (long it = 0; it < a.pass_bound; ++it) {
        // ---- refill: lanes without a ray take the next ones from the queue; rays that miss the aabb are written at once
        for (int tries = 0; tries < 1024; ++tries) {
            const bool need = !active && !exhausted;
            unsigned long long r = 0;
            if (!march_take(queue, need, lane, r)) break;
            if (need) {
                if (r >= (unsigned long long)a.n_rays) exhausted = true;
                else {
                    ray = (long)r;
#pragma unroll
                    for (int k = 0; k < 3; ++k) { o[k] = a.origins[ray * 3 + k]; d[k] = a.dirs[ray * 3 + k]; }
                    const bool hit = render_ray_interval(o, d, a.scene, a.near, a.far, tmin, tmax);
                    if (a.jitter) tmin += a.jitter[ray] * a.dt;             // stratified marching (training): t_min + u dt, u in [0,1) per ray
                    const float acc0[3] = {0.f, 0.f, 0.f};
                    if (!hit || !(tmin < tmax)) render_write(a, ray, acc0, 0.f, 0.f);
                    else {
                        active = true; n = 0; T_all = 1.f; T_s = 1.f; opac = 0.f; dep = 0.f;
                        acc[0] = acc[1] = acc[2] = 0.f;
                        n_lim = (int)fminf(ceilf((tmax - tmin) / a.dt) + 1.f, (float)a.n_max);      // (a.n_max <= 1e8 + 2: the conversion cannot overflow)
                        render_sh4_f16(d, sh2);
                    }
                }
            }
        }
        if (!__any(active)) {
            if (__all(exhausted)) { finished = true; break; }        // the queue is empty and nothing is in flight
            continue;                                                // (a long run of missed rays used up this pass's refill rounds)
        }
        // ---- advance every live ray to its next lattice sample inside an occupied cell
        float x[3] = {0.f, 0.f, 0.f}, tm = 0.f;
        const bool was_active = active;
        if (active && n >= n_lim) active = false;                   // (never taken: t_mid >= t_max ends a ray first; the argument-derived bound per ray)
        const bool have = march_advance(g, o, d, tmin, tmax, a.dt, n, active, x, &tm, 4096);
        if (was_active && !active) render_write(a, ray, acc, opac, dep);       // left [t_min, t_max)
        if (!__any(have)) continue;
        // ---- density of the wave's samples; their features land in the colour net's input rows
        const bool inside_m = march_density<true>(have, x, a.model, a.lv, a.table, dw, sX, sH, sOut, lane);
        bool surv = false;
        float w = 0.f;
        if (have) {
            // march_composite and march_color_row with omega = 1, kept local: through the helpers the training forward of this kernel measured
            // ~2 % slower (the arithmetic is theirs operation for operation: tests/test_hip_render_pair.py holds the two kernels equal bit for bit)
            const float sigma = inside_m ? __expf(sOut[lane] - 1.f) : 0.f;
            const float alpha = 1.f - __expf(-sigma * a.dt);
            surv = T_all >= a.eps && (a.alpha_thre <= 0.f || alpha >= a.alpha_thre);
            T_all *= (1.f - alpha);
            ++n;
            if (surv) {
                w = alpha * T_s;
                T_s *= (1.f - alpha);
                uint32_t* xr = reinterpret_cast<uint32_t*>(sX + lane * NGP_XRS);
#pragma unroll
                for (int j = 0; j < 8; ++j) xr[j] = sh2[j];
                reinterpret_cast<_Float16*>(sX + lane * NGP_XRS)[31] = (_Float16)1.f;
            }
        }
        if (__any(surv)) {
            // ---- colour of the surviving samples: X = (fp16 SH4(d) | 15 features | 1) -> relu 64 -> relu 64 -> 3, sigmoid (as ngp_rgb_kernel)
            march_color(sX, sH, sH, sO, cw1f, a.cw2, cw3f, lane);
            if (surv) {
                const float4 pre = *reinterpret_cast<const float4*>(sO + lane * 4);
                const float pv[3] = {pre.x, pre.y, pre.z};
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) acc[ch] += w * march_sigmoid_f16(pv[ch]);
                opac += w;
                dep += w * tm;
                ++my_samples;
            }
        }
        if (have && T_all < a.eps) { active = false; render_write(a, ray, acc, opac, dep); }    // transmittance below early_stop_eps: the ray ends
        wave_sync();
    }
    // the survivors this wave composited: one atomic per wave
    unsigned long long tot = my_samples;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off, 64);
    if (lane == 0 && tot) atomicAdd(a.n_samples, tot);
    // the bound was reached with rays still queued or in flight: say so in bit 63 of the ray counter (dreg_nerf_amd/render.py raises)
    if (!finished && lane == 0) atomicOr(a.queue, 1ull << 63);
}

static int render_launch(const float* origins, const float* viewdirs, const float* jitter, long n_rays, const uint8_t* binary, int rx, int ry, int rz,
                         const uint32_t* coarse_bits, const void* table, const void* w1, const void* w2, const void* cw1, const void* cw2, const void* cw3,
                         const uint32_t* offset, const uint32_t* size, const uint32_t* res, const float* scale, const uint32_t* hashed,
                         const float* roi_aabb, const float* scene_aabb, const float* model_aabb, float near_plane, float far_plane,
                         float render_step_size, float alpha_thre, float early_stop_eps, const float* bkgd,
                         float* rgb, float* opacity, float* depth, unsigned long long* n_samples, void* queue, void* stream)
{
    if (n_rays < 0) return DREG_EINVAL;
    if (n_rays == 0) return DREG_OK;
    if (!origins || !viewdirs || !bkgd || !rgb || !opacity || !depth || !n_samples || !queue) return DREG_EINVAL;
    RenderArgs a;
    if (march_fill_block(a, binary, rx, ry, rz, coarse_bits, table, w1, w2, true, cw1, cw2, cw3, offset, size, res, scale, hashed,
                         roi_aabb, scene_aabb, model_aabb, near_plane, far_plane, render_step_size, alpha_thre, true) != DREG_OK)
        return DREG_EINVAL;
    a.origins = origins; a.dirs = viewdirs; a.jitter = jitter; a.n_rays = n_rays;
    a.eps = early_stop_eps;
    for (int k = 0; k < 3; ++k) a.bkgd[k] = bkgd[k];
    a.pass_bound = march_pass_bound(n_rays, (double)(a.n_max + 2));
    a.rgb = rgb; a.opacity = opacity; a.depth = depth; a.n_samples = n_samples; a.queue = (unsigned long long*)queue;
    long waves = (n_rays + 63) / 64;
    if (waves > g_render_waves) waves = g_render_waves;
    hipLaunchKernelGGL(ngp_render_kernel, dim3((unsigned)waves), dim3(64), 0, (hipStream_t)stream, a);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

extern "C" {

// Render n_rays rays of one block.  Caller-owned device buffers: origins / viewdirs fp32 [N,3], binary uint8 [rx,ry,rz], coarse_bits (optional),
// the fp16 inference copies (table / w1 / w2 of mlp_base.params, cw1 / cw2 / cw3 of color_mlp.params), rgb fp32 [N,3], opacity / depth fp32 [N],
// n_samples: one u64 and queue: 8 bytes, both zeroed by the caller on `stream`.  Level arrays, aabbs and bkgd are HOST pointers.
int dreg_ngp_render(const float* origins, const float* viewdirs, long n_rays, const uint8_t* binary, int rx, int ry, int rz, const uint32_t* coarse_bits,
                    const void* table, const void* w1, const void* w2, const void* cw1, const void* cw2, const void* cw3,
                    const uint32_t* offset, const uint32_t* size, const uint32_t* res, const float* scale, const uint32_t* hashed,
                    const float* roi_aabb, const float* scene_aabb, const float* model_aabb, float near_plane, float far_plane,
                    float render_step_size, float alpha_thre, float early_stop_eps, const float* bkgd,
                    float* rgb, float* opacity, float* depth, unsigned long long* n_samples, void* queue, void* stream)
{
    return render_launch(origins, viewdirs, nullptr, n_rays, binary, rx, ry, rz, coarse_bits, table, w1, w2, cw1, cw2, cw3, offset, size, res, scale, hashed,
                         roi_aabb, scene_aabb, model_aabb, near_plane, far_plane, render_step_size, alpha_thre, early_stop_eps, bkgd,
                         rgb, opacity, depth, n_samples, queue, stream);
}

// dreg_ngp_render with stratified marching (the training forward): ray i starts at t_min + jitter[i] * render_step_size, jitter fp32 [N] in [0,1)
// on the device.  With jitter == 0 the results equal dreg_ngp_render's bit for bit.
int dreg_ngp_render_train(const float* origins, const float* viewdirs, const float* jitter, long n_rays, const uint8_t* binary, int rx, int ry, int rz,
                          const uint32_t* coarse_bits, const void* table, const void* w1, const void* w2, const void* cw1, const void* cw2, const void* cw3,
                          const uint32_t* offset, const uint32_t* size, const uint32_t* res, const float* scale, const uint32_t* hashed,
                          const float* roi_aabb, const float* scene_aabb, const float* model_aabb, float near_plane, float far_plane,
                          float render_step_size, float alpha_thre, float early_stop_eps, const float* bkgd,
                          float* rgb, float* opacity, float* depth, unsigned long long* n_samples, void* queue, void* stream)
{
    if (!jitter && n_rays > 0) return DREG_EINVAL;
    return render_launch(origins, viewdirs, jitter, n_rays, binary, rx, ry, rz, coarse_bits, table, w1, w2, cw1, cw2, cw3, offset, size, res, scale, hashed,
                         roi_aabb, scene_aabb, model_aabb, near_plane, far_plane, render_step_size, alpha_thre, early_stop_eps, bkgd,
                         rgb, opacity, depth, n_samples, queue, stream);
}

#ifdef DREG_PROBE
void dreg_render_set_waves(int n) { g_render_waves = n > 0 ? n : 2048; }
#endif

}  // extern "C"
