// Surface-field visibility of query points from a NeRF block's training cameras (row N1 of SURVEY.md §8f), gfx950.
//
// Replaces, in ONE kernel, the reference's chain for every (camera, point) ray
//   nerfacc.ray_aabb_intersect -> nerfacc _C.ray_marching (two passes, sample list in HBM) -> tcnn density at every sample ->
//   CUB segmented exclusive cumprod (transmittance) -> torch_scatter.scatter_max(alpha*T) -> >= cut_off -> max over cameras
//   (conerf/utils/nerfacc_utils.py:84-222, conerf/loss/confidence_loss.py:56-160, conerf/register/sample_grid.py:244-318).
// One lane = one ray, 64 rays per wave march in lock step: every lane advances to its next lattice sample
// t_mid = t_min + (n + 1/2) dt that falls in an occupied cell of the 128^3 binary grid (empty cells are skipped to the
// cell's exit, as nerfacc does), the wave evaluates the 64 densities together (hash-grid gather per lane, 32->64->16 MLP on
// fp16 MFMA through LDS: march_density over ngp_field.h), then each lane updates T and max(alpha*T).  Only the binary label is
// needed, so a ray stops as soon as the label is decided: hit (max >= cut_off), or T < max(cut_off, early_stop_eps)
// (alpha*T <= T can no longer reach cut_off) — no sample list, no later samples evaluated.  Labels of a point are OR-ed
// over cameras with one atomic per hit.  nerfacc 0.3.5 / tcnn are absent from the reference tree: parity unpinned.
#include "march.h"      // the lattice advance and the density of a wave's samples, shared with render.hip (field: ngp_field.h)
#include <cstring>
struct VisArgs : MarchBlock {   // the block (march.h; no colour net, no near / far, no n_max), then the launch's own
    const float* cams;     // [Nc,3] camera centres
    const float* pts;      // [Np,3]
    int* label;            // [Np] OR over cameras
    int Nc, Np;
    float cut_off, early_eps;
    int max_steps;
    unsigned long long* queue;   // persistent forms: this block's ray counter (zeroed by the caller)
};

// The ray from camera c to point p: origin o, unit direction d, t_max = their distance, t_min from the slab test against the scene aabb
// (marching starts at max(near, 0)).  Returns whether there is anything to march.
__device__ __forceinline__ bool vis_ray_setup(const VisArgs& a, int c, int p, float (&o)[3], float (&d)[3], float& tmin, float& tmax)
{
    float n2 = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[k] = a.cams[c * 3 + k]; d[k] = a.pts[(long)p * 3 + k] - o[k]; n2 += d[k] * d[k]; }
    tmax = sqrtf(n2);
    const float inv = tmax > 0.f ? 1.f / tmax : 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] *= inv;
    float near = -1e30f, far = 1e30f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float id = 1.f / d[k];
        float t0 = (a.scene[k] - o[k]) * id, t1 = (a.scene[3 + k] - o[k]) * id;
        if (t0 > t1) { const float tt = t0; t0 = t1; t1 = tt; }
        near = fmaxf(near, t0); far = fminf(far, t1);
    }
    tmin = fmaxf(near, 0.f);
    return (near <= far) && far > 0.f && tmax > 0.f;
}

// The lock-step launch: the plain statement of the labels, which the persistent form below (queue, refill, coarse-cell skip, march_advance)
// is tested against — so it keeps its OWN advance loop and transmittance update, and shares only the density of a sample (march_density).
__global__ __launch_bounds__(64) void surface_visibility_kernel(VisArgs a)
{
    __shared__ __attribute__((aligned(16))) char smem[64 * NGP_XRS + 64 * NGP_HRS + 64 * 4];
    char* sX = smem;
    char* sH = sX + 64 * NGP_XRS;
    float* sOut = reinterpret_cast<float*>(sH + 64 * NGP_HRS);
    const int lane = threadIdx.x;
    const long ray = (long)blockIdx.x * 64 + lane;
    const long nrays = (long)a.Nc * a.Np;
    bool done = ray >= nrays;
    const int c = done ? 0 : (int)(ray / a.Np), p = done ? 0 : (int)(ray - (long)c * a.Np);
    float o[3], d[3], tmax = 0.f, tmin = 0.f;
    if (!vis_ray_setup(a, c, p, o, d, tmin, tmax)) done = true;
    float T = 1.f, best = 0.f;
    int n = 0;
    const float roi_ext[3] = {a.roi[3] - a.roi[0], a.roi[4] - a.roi[1], a.roi[5] - a.roi[2]};
    const int rdim[3] = {a.rx, a.ry, a.rz};
    const float stop_T = fmaxf(a.cut_off, a.early_eps);
    NgpDensityW dw;
    ngp_load_density_w(dw, a.w1, a.w2, lane);

    for (int iter = 0; iter < a.max_steps; ++iter) {
        // ---- advance to the next lattice sample inside an occupied cell
        bool have = false;
        float x[3] = {0.f, 0.f, 0.f};
        for (int guard = 0; !done && !have && guard < 4096; ++guard) {
            const float tm = tmin + ((float)n + 0.5f) * a.dt;
            if (tm >= tmax) { done = true; break; }
            float u[3];
            bool inside = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) { x[k] = o[k] + tm * d[k]; u[k] = (x[k] - a.roi[k]) / roi_ext[k]; inside = inside && u[k] >= 0.f && u[k] <= 1.f; }
            int ci[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) ci[k] = min(max((int)floorf(u[k] * (float)rdim[k]), 0), rdim[k] - 1);
            const bool occ = inside && a.binary[((long)ci[0] * a.ry + ci[1]) * a.rz + ci[2]] != 0;
            if (occ) { have = true; break; }
            // skip to the exit of this cell (or, outside the roi, just step): only lattice points that stay in the cell whatever the rounding
            // (march.h: the contract of the skip and its allowance, march_face_slack / march_steps_to_face)
            float steps = 1e9f;
            if (inside) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (d[k] != 0.f) {
                        const float face = a.roi[k] + (float)(ci[k] + (d[k] > 0.f ? 1 : 0)) * roi_ext[k] / (float)rdim[k];
                        steps = fminf(steps, march_steps_to_face(fabsf(face - x[k]), march_face_slack(o[k], a.roi[k], a.roi[3 + k]), d[k], a.dt));
                    }
                }
            } else steps = 0.f;
            n += 1 + max((int)floorf(steps), 0);
        }
        if (!__any(have)) break;
        // ---- density of the 64 samples
        const bool inside_m = march_density<false>(have, x, a.model, a.lv, a.table, dw, sX, sH, sOut, lane);
        if (have) {
            const float sigma = inside_m ? __expf(sOut[lane] - 1.f) : 0.f;
            const float alpha = 1.f - __expf(-sigma * a.dt);
            const bool vis = T >= a.early_eps && (a.alpha_thre <= 0.f || alpha >= a.alpha_thre);
            if (vis) best = fmaxf(best, alpha * T);
            T *= (1.f - alpha);
            ++n;
            if (best >= a.cut_off || T < stop_T) done = true;
        }
        wave_sync();
    }
    if (ray < nrays && best >= a.cut_off) atomicOr(a.label + p, 1);
}

// ------------------------------------------------------------------------------------------------
// Persistent form (round 3).  The lock-step kernel above gives every wave 64 rays and runs until the LONGEST of them is decided: the
// others' lanes idle through the hash-grid gathers and the MLP of every remaining iteration, and a point already seen from one camera
// is marched from all the others.  Here a wave keeps its 64 lanes full: a lane whose ray is decided takes the next ray from a queue
// (one atomic per wave and refill), and a ray whose point already carries the label is not marched at all (rays are queued camera by
// camera, so the later cameras mostly find the label set).  Per-ray arithmetic is unchanged: the labels are the same.
#ifdef DREG_PROBE
__device__ long g_pass_bound = 1L << 22;   // passes of the march loop per wave (test hook of the measurement build: dreg_visibility_set_pass_bound)
#else
static constexpr long g_pass_bound = 1L << 22;
#endif
__device__ __forceinline__ void vis_march_queue(const VisArgs& a, unsigned long long* __restrict__ queue)
{
    __shared__ __attribute__((aligned(16))) char smem[64 * NGP_XRS + 64 * NGP_HRS + 64 * 4];
    char* sX = smem;
    char* sH = sX + 64 * NGP_XRS;
    float* sOut = reinterpret_cast<float*>(sH + 64 * NGP_HRS);
    const int lane = threadIdx.x;
    // the coarse occupancy (one bit per 4^3 cells) in LDS: a ray walks the empty space of a block — from the aabb's face to the surface —
    // in coarse cells looked up here (~100 cycles) instead of fine cells looked up in global memory (a dependent load of 1-2 us each);
    // every pass of the loop below waits for its slowest lane, and a freshly queued ray's walk WAS that lane
    __shared__ uint32_t sCoarse[1024];
    const unsigned long long nrays = (unsigned long long)a.Nc * (unsigned long long)a.Np;
    if (nrays == 0) return;                                       // (a block without rays: its descriptor holds no pointers, dreg_surface_visibility_fill_desc)
    march_load_coarse(sCoarse, a, lane);
    __syncthreads();
    MarchGrid g;
    march_grid(g, a, sCoarse);
    MarchQueue rays = {queue};
    const float stop_T = fmaxf(a.cut_off, a.early_eps);
    NgpDensityW dw;
    ngp_load_density_w(dw, a.w1, a.w2, lane);

    // per-lane ray state
    bool active = false, exhausted = false;
    int p = 0, n = 0;
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f}, tmax = 0.f, tmin = 0.f, T = 1.f, best = 0.f;

    bool finished = false;
    const long pass_bound = g_pass_bound;
    for (long it = 0; it < pass_bound; ++it) {                    // (bound: a safety net, never reached — every pass advances every live ray)
        // ---- refill: lanes without a ray take the next ones from the queue, skipping rays whose point is already labelled
        for (int tries = 0; tries < 1024; ++tries) {
            const bool need = !active && !exhausted;
            unsigned long long ray = 0;
            if (!march_take(rays, need, lane, ray)) break;
            if (need) {
                if (ray >= nrays) exhausted = true;
                else {
                    const int c = (int)(ray / (unsigned long long)a.Np);
                    p = (int)(ray - (unsigned long long)c * (unsigned long long)a.Np);
                    if (__hip_atomic_load(a.label + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {      // not yet seen from an earlier camera (device-scope load: other waves set it)
                        if (vis_ray_setup(a, c, p, o, d, tmin, tmax)) { active = true; T = 1.f; best = 0.f; n = 0; }
                    }
                }
            }
        }
        if (!__any(active)) {
            if (__all(exhausted)) { finished = true; break; }        // the queue is empty and nothing is in flight
            continue;                                                // (a long run of skipped rays used up this pass's refill rounds)
        }
        // ---- advance every live ray to its next lattice sample inside an occupied cell
        float x[3] = {0.f, 0.f, 0.f};
        const bool have = march_advance(g, o, d, tmin, tmax, a.dt, n, active, x, nullptr, 4096);
        if (!__any(have)) continue;
        // ---- density of the 64 samples
        const bool inside_m = march_density<false>(have, x, a.model, a.lv, a.table, dw, sX, sH, sOut, lane);
        if (have) {
            const float sigma = inside_m ? __expf(sOut[lane] - 1.f) : 0.f;
            const float alpha = 1.f - __expf(-sigma * a.dt);
            const bool vis = T >= a.early_eps && (a.alpha_thre <= 0.f || alpha >= a.alpha_thre);
            if (vis) best = fmaxf(best, alpha * T);
            T *= (1.f - alpha);
            ++n;
            if (best >= a.cut_off) { atomicOr(a.label + p, 1); active = false; }
            else if (T < stop_T) active = false;
            // another camera's ray may have labelled this point in the meantime: its label is decided, this ray need not finish (a call's
            // duration is its LONGEST ray — typically a camera on the far side marching through the whole block — not its average one)
            else if ((it & 3) == 3 && __hip_atomic_load(a.label + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) active = false;
        }
        wave_sync();
    }
    // the bound was reached with rays still queued or in flight: their points stay unlabelled — say so in bit 63 of the ray counter
    // (the caller reads it back: dreg_nerf_amd/visibility.py raises on the next call)
    if (!finished && lane == 0) atomicOr(queue, 1ull << 63);
}

__global__ __launch_bounds__(64) void surface_visibility_persistent_kernel(VisArgs a, unsigned long long* __restrict__ queue)
{
    vis_march_queue(a, queue);
}
// Several blocks in ONE launch (a training step asks for the labels of 8 blocks: one pair of point sets each).  A call's duration is
// its longest ray, not its average one, so eight launches cost eight tails; here every wave works through ALL blocks' queues, starting at
// block (workgroup index mod n): the blocks' tails overlap.  A wave serves one block at a time (its MLP weights live in registers).
__global__ __launch_bounds__(64) void surface_visibility_multi_kernel(const VisArgs* __restrict__ descs, int n)
{
    for (int i = 0; i < n; ++i) {
        const int b = ((int)blockIdx.x + i) % n;
        vis_march_queue(descs[b], descs[b].queue);
        __syncthreads();
    }
}

// one bit per 4^3 block of the occupancy volume: set when any of its cells is occupied (bits must be zeroed by the caller)
__global__ void occupancy_coarse_bits_kernel(const uint8_t* __restrict__ binary, uint32_t* __restrict__ bits, int rx, int ry, int rz, int cx, int cy, int cz)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= cx * cy * cz) return;
    const int z0 = (b % cz) * 4, y0 = ((b / cz) % cy) * 4, x0 = (b / (cz * cy)) * 4;
    bool any = false;
    for (int dx = 0; dx < 4 && x0 + dx < rx; ++dx)
        for (int dy = 0; dy < 4 && y0 + dy < ry; ++dy)
            for (int dz = 0; dz < 4 && z0 + dz < rz; ++dz) any = any || binary[((long)(x0 + dx) * ry + y0 + dy) * rz + z0 + dz] != 0;
    if (any) atomicOr(bits + (b >> 5), 1u << (b & 31));
}

extern "C" {

// bits: uint32 [ceil(ceil(rx/4) * ceil(ry/4) * ceil(rz/4) / 32)], zeroed by the caller; bit ((x/4) * cy + y/4) * cz + z/4
int dreg_occupancy_coarse_bits(const uint8_t* binary, uint32_t* bits, int rx, int ry, int rz, void* stream)
{
    const int cx = (rx + 3) / 4, cy = (ry + 3) / 4, cz = (rz + 3) / 4;
    if (!binary || !bits) return DREG_EINVAL;
    hipLaunchKernelGGL(occupancy_coarse_bits_kernel, dim3((cx * cy * cz + 255) / 256), dim3(256), 0, (hipStream_t)stream, binary, bits, rx, ry, rz, cx, cy, cz);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

// One block's descriptor from an entry point's arguments, validated as the renderers validate theirs (march_fill_block): DREG_EINVAL, with
// nothing launched, for a null pointer, an empty grid or a step that is not > 0 (the persistent kernel would spin to its pass bound on dt <= 0).
static int vis_fill(VisArgs& a, const float* cams, const float* pts, const uint8_t* binary, int* label, const void* table, const void* w1, const void* w2,
                    const uint32_t* offset, const uint32_t* size, const uint32_t* res, const float* scale, const uint32_t* hashed,
                    const float* roi_aabb, const float* scene_aabb, const float* model_aabb, int rx, int ry, int rz, int Nc, int Np,
                    float render_step_size, float cut_off, float early_stop_eps, float alpha_thre, void* queue, const uint32_t* coarse_bits)
{
    if (!cams || !pts || !label || Nc < 0 || Np < 0) return DREG_EINVAL;
    a.cams = cams; a.pts = pts; a.label = label; a.Nc = Nc; a.Np = Np;
    a.cut_off = cut_off; a.early_eps = early_stop_eps;
    a.max_steps = 1 << 16;
    a.queue = (unsigned long long*)queue;
    return march_fill_block(a, binary, rx, ry, rz, coarse_bits, table, w1, w2, false, nullptr, nullptr, nullptr, offset, size, res, scale, hashed,
                            roi_aabb, scene_aabb, model_aabb, -INFINITY, INFINITY, render_step_size, alpha_thre, false);
}
// label[p] = OR over cameras of (max_samples alpha*T >= cut_off) along the ray camera -> point p (must be zeroed by the caller).
// table/w1/w2: fp16 inference copies of mlp_base.params; level arrays / aabbs are HOST pointers (16 entries / 6 floats).
int dreg_surface_visibility(const float* cams, const float* pts, const uint8_t* binary, int* label,
                            const void* table, const void* w1, const void* w2,
                            const uint32_t* offset, const uint32_t* size, const uint32_t* res, const float* scale, const uint32_t* hashed,
                            const float* roi_aabb, const float* scene_aabb, const float* model_aabb,
                            int rx, int ry, int rz, int Nc, int Np, float render_step_size, float cut_off, float early_stop_eps,
                            float alpha_thre, void* stream)
{
    if ((long)Nc * Np == 0) return DREG_OK;
    VisArgs a;
    if (vis_fill(a, cams, pts, binary, label, table, w1, w2, offset, size, res, scale, hashed, roi_aabb, scene_aabb, model_aabb, rx, ry, rz, Nc, Np,
                 render_step_size, cut_off, early_stop_eps, alpha_thre, nullptr, nullptr) != DREG_OK)
        return DREG_EINVAL;
    const long nrays = (long)Nc * Np;
    hipLaunchKernelGGL(surface_visibility_kernel, dim3((unsigned)((nrays + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}
// Descriptor-table form for several blocks per launch.  The caller owns the table: n records of dreg_surface_visibility_desc_bytes() bytes,
// filled ON THE HOST by dreg_surface_visibility_fill_desc (same arguments as dreg_surface_visibility_queue, one block each), copied to
// the device by the caller, then passed to dreg_surface_visibility_multi.  Labels / queues of every block zeroed by the caller.
size_t dreg_surface_visibility_desc_bytes() { return sizeof(VisArgs); }
int dreg_surface_visibility_fill_desc(void* host_desc, const float* cams, const float* pts, const uint8_t* binary, int* label,
                                      const void* table, const void* w1, const void* w2,
                                      const uint32_t* offset, const uint32_t* size, const uint32_t* res, const float* scale, const uint32_t* hashed,
                                      const float* roi_aabb, const float* scene_aabb, const float* model_aabb,
                                      int rx, int ry, int rz, int Nc, int Np, float render_step_size, float cut_off, float early_stop_eps,
                                      float alpha_thre, void* queue, const uint32_t* coarse_bits)
{
    if (!host_desc || !queue) return DREG_EINVAL;
    VisArgs a;
    if ((long)Nc * Np == 0) memset(&a, 0, sizeof(a));            // no rays: the kernel returns before it reads anything else of the descriptor
    else if (vis_fill(a, cams, pts, binary, label, table, w1, w2, offset, size, res, scale, hashed, roi_aabb, scene_aabb, model_aabb, rx, ry, rz, Nc, Np,
                      render_step_size, cut_off, early_stop_eps, alpha_thre, queue, coarse_bits) != DREG_OK)
        return DREG_EINVAL;
    memcpy(host_desc, &a, sizeof(a));
    return DREG_OK;
}
DREG_KNOB(int, g_vis_waves, 4096);        // tuning (include/dreg_nerf_probe.h): one-wave workgroups of the persistent launches (256 CUs x 16)
// max_waves (0 = the default 4096 = 16 per CU): one-wave workgroups of the persistent launch.  A workgroup holds 18.7 KB of LDS for as long as the launch
// runs, so a full-width launch leaves a CU's LDS to nobody else; a BACKGROUND launch — the training step's gradient-free 'tilde' labels, marched on a side
// stream while backward runs (train_step.TrainStep.split_labels) — asks for one or two waves per CU and takes proportionally longer.  Same labels.
int dreg_surface_visibility_multi_waves(const void* descs_dev, int n, long total_rays, int max_waves, void* stream)
{
    if (n <= 0 || total_rays <= 0) return DREG_OK;
    if (!descs_dev || max_waves < 0) return DREG_EINVAL;
    long waves = (total_rays + 63) / 64;
    if (waves > g_vis_waves) waves = g_vis_waves;
    if (max_waves > 0 && waves > max_waves) waves = max_waves;
    hipLaunchKernelGGL(surface_visibility_multi_kernel, dim3((unsigned)waves), dim3(64), 0, (hipStream_t)stream, (const VisArgs*)descs_dev, n);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}
int dreg_surface_visibility_multi(const void* descs_dev, int n, long total_rays, void* stream)
{
    return dreg_surface_visibility_multi_waves(descs_dev, n, total_rays, 0, stream);
}
// The same labels from the persistent kernel (lanes refilled from a ray queue; rays of points that already carry the label are not
// marched).  queue: 8 bytes of device memory the CALLER has zeroed on this stream (the ray counter).
#ifdef DREG_PROBE
void dreg_visibility_set_waves(int n) { g_vis_waves = n > 0 ? n : 4096; }
// Test hook: passes of the persistent kernels' march loop per wave (0 = the default 2^22, never reached by a real extraction).  A launch
// that hits the bound sets bit 63 of its ray counter(s) — the caller's `queue` words — instead of silently leaving points unlabelled.
int dreg_visibility_set_pass_bound(long passes)
{
    const long v = passes > 0 ? passes : (1L << 22);
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_pass_bound), &v, sizeof(v));
}
#endif
int dreg_surface_visibility_queue(const float* cams, const float* pts, const uint8_t* binary, int* label,
                                  const void* table, const void* w1, const void* w2,
                                  const uint32_t* offset, const uint32_t* size, const uint32_t* res, const float* scale, const uint32_t* hashed,
                                  const float* roi_aabb, const float* scene_aabb, const float* model_aabb,
                                  int rx, int ry, int rz, int Nc, int Np, float render_step_size, float cut_off, float early_stop_eps,
                                  float alpha_thre, void* queue, const uint32_t* coarse_bits, void* stream)
{
    if ((long)Nc * Np == 0) return DREG_OK;
    if (!queue) return DREG_EINVAL;
    VisArgs a;
    if (vis_fill(a, cams, pts, binary, label, table, w1, w2, offset, size, res, scale, hashed, roi_aabb, scene_aabb, model_aabb, rx, ry, rz, Nc, Np,
                 render_step_size, cut_off, early_stop_eps, alpha_thre, queue, coarse_bits) != DREG_OK)
        return DREG_EINVAL;
    const long nrays = (long)Nc * Np;
    long waves = (nrays + 63) / 64;
    if (waves > g_vis_waves) waves = g_vis_waves;
    hipLaunchKernelGGL(surface_visibility_persistent_kernel, dim3((unsigned)waves), dim3(64), 0, (hipStream_t)stream, a, (unsigned long long*)queue);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

}  // extern "C"
