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
//
// The kernel, its arguments and its launch are render_loop.h's (ngp_render_kernel<false>, render_launch<false>), which the recording training
// forward of render_samples.hip instantiates a second time; this file holds the two entry points of the plain form.
#include "render_loop.h"
#include "../../include/dreg_nerf.h"   // signature check of the entry point defined here

DREG_KNOB(int, g_render_waves, 2048);     // tuning (include/dreg_nerf_probe.h): one-wave workgroups of the launch (256 CUs x 8: 19.7 KB of LDS each)

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
    return render_launch<false>(origins, viewdirs, nullptr, n_rays, binary, rx, ry, rz, coarse_bits, table, w1, w2, cw1, cw2, cw3, offset, size, res, scale, hashed,
                                roi_aabb, scene_aabb, model_aabb, near_plane, far_plane, render_step_size, alpha_thre, early_stop_eps, bkgd,
                                rgb, opacity, depth, n_samples, queue, g_render_waves, nullptr, stream);
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
    return render_launch<false>(origins, viewdirs, jitter, n_rays, binary, rx, ry, rz, coarse_bits, table, w1, w2, cw1, cw2, cw3, offset, size, res, scale, hashed,
                                roi_aabb, scene_aabb, model_aabb, near_plane, far_plane, render_step_size, alpha_thre, early_stop_eps, bkgd,
                                rgb, opacity, depth, n_samples, queue, g_render_waves, nullptr, stream);
}

#ifdef DREG_PROBE
void dreg_render_set_waves(int n) { g_render_waves = n > 0 ? n : 2048; }
#endif

}  // extern "C"
