// Training of one NeRF block on a SAMPLE LIST (gfx950), rule in DESIGN.md §3o: the training forward of render.hip that writes its surviving
// samples down, and the kernel that turns per-ray upstream gradients (colour, opacity, depth) into the per-sample dL/dsigma and dL/dc that
// dreg_ngp_points_bwd (field_train.hip) takes.  fp64 restatement: tests/render_samples_restatement.py.
//
// The forward is ngp_render_kernel<true> of render_loop.h: the loop of dreg_ngp_render_train itself, instantiated with the record store, so
// rgb, opacity, depth and n_samples are those of dreg_ngp_render_train bit for bit by construction.  Per survivor k of a ray it records, fp32 as
// the lane holds them (nothing is recomputed):
//   ray, ord        the ray and the number of earlier survivors of it
//   t, x[3]         t_mid and the position march_advance returned
//   T_next, w       T_s after the sample (T_{k+1}) and the weight
//   c[3]            the three fp16 sigmoid colours as float
//   P[3], Pd        acc and dep after the sample (sum_{j<=k} w_j c_j, sum_{j<=k} w_j t_j)
// A pass's survivors take consecutive slots from one counter: ballot, popc, lane rank, one returning atomic per wave and pass (MarchQueue's
// shape).  A survivor whose slot is >= capacity is not written (every store is guarded) and the counter keeps counting, so the caller learns the
// true count; the per-ray outputs do not depend on the capacity.  The list's ORDER depends on the scheduling: callers sort it by (ray, ord).
//
// ngp_samples_grad_kernel, one lane per record, any order.  C, O, D: the forward's rgb (background included), opacity and depth of the ray,
// g_C, g_O, g_D the upstream gradients (each may be absent = zeros):
//   dL/dc_k     = w_k g_C
//   dL/dsigma_k = dt ( sum_ch g_C[ch] (T_{k+1} c_k[ch] - (C[ch] - P_k[ch]))  +  g_O (1 - O)  +  g_D (T_{k+1} t_k - (D - Pd_k)) )
// (dw_k/dsigma_k = dt T_{k+1}, dw_j/dsigma_k = -dt w_j for j > k, dO/dsigma_k = dt T_end = dt (1 - O); the colour term is §3c's, in the order
// ngp_render_bwd_kernel evaluates it), and dirs_k = viewdirs[ray]: with x these are dreg_ngp_points_bwd's four inputs.
#include "render_loop.h"
#include "../../include/dreg_nerf.h"   // signature check of the entry points defined here

DREG_KNOB(int, g_render_samples_waves, 2048);     // tuning (include/dreg_nerf_probe.h): one-wave workgroups of the launch; same per-ray results and same sorted list at every width

struct SamplesGradArgs {
    long n;
    const int* ray;
    const float *t, *T_next, *w, *c, *P, *Pd;
    const float *viewdirs, *rgb, *opacity, *depth;
    const float *g_rgb, *g_opacity, *g_depth;      // each may be null (zeros)
    float dt;
    float *dirs, *g_sigma, *g_c;
};

__global__ __launch_bounds__(256) void ngp_samples_grad_kernel(SamplesGradArgs a)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const long r = a.ray[i];
    const float T = a.T_next[i], w = a.w[i];
    float dsig = 0.f;
    float gc[3] = {0.f, 0.f, 0.f};
    if (a.g_rgb) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float gr = a.g_rgb[r * 3 + ch];
            dsig += gr * (T * a.c[i * 3 + ch] - (a.rgb[r * 3 + ch] - a.P[i * 3 + ch]));
            gc[ch] = w * gr;
        }
    }
    if (a.g_opacity) dsig += a.g_opacity[r] * (1.f - a.opacity[r]);
    if (a.g_depth) dsig += a.g_depth[r] * (T * a.t[i] - (a.depth[r] - a.Pd[i]));
    a.g_sigma[i] = a.dt * dsig;
#pragma unroll
    for (int k = 0; k < 3; ++k) { a.g_c[i * 3 + k] = gc[k]; a.dirs[i * 3 + k] = a.viewdirs[r * 3 + k]; }
}

extern "C" {

// dreg_ngp_render_train that also writes the list of its surviving samples.  The arguments of dreg_ngp_render_train, then: capacity (records the
// caller's arrays hold, >= 0), the record arrays (device; int32 s_ray / s_ord [capacity], fp32 s_t [capacity], s_x [capacity,3], s_T_next / s_w
// [capacity], s_c / s_P [capacity,3], s_Pd [capacity]; all required when capacity > 0) and slots: one u64 zeroed by the caller on `stream`, on
// return the TRUE number of survivors (= *n_samples), whatever the capacity.  Records whose slot is >= capacity are not written.
int dreg_ngp_render_train_samples(const float* origins, const float* viewdirs, const float* jitter, long n_rays, const uint8_t* binary, int rx, int ry, int rz,
                                  const uint32_t* coarse_bits, const void* table, const void* w1, const void* w2, const void* cw1, const void* cw2, const void* cw3,
                                  const uint32_t* offset, const uint32_t* size, const uint32_t* res, const float* scale, const uint32_t* hashed,
                                  const float* roi_aabb, const float* scene_aabb, const float* model_aabb, float near_plane, float far_plane,
                                  float render_step_size, float alpha_thre, float early_stop_eps, const float* bkgd,
                                  float* rgb, float* opacity, float* depth, unsigned long long* n_samples, void* queue,
                                  long capacity, int* s_ray, int* s_ord, float* s_t, float* s_x, float* s_T_next, float* s_w, float* s_c, float* s_P, float* s_Pd,
                                  void* slots, void* stream)
{
    if (n_rays < 0) return DREG_EINVAL;
    if (n_rays == 0) return DREG_OK;
    if (capacity < 0) return DREG_EINVAL;
    if (capacity > 0 && (!s_ray || !s_ord || !s_t || !s_x || !s_T_next || !s_w || !s_c || !s_P || !s_Pd)) return DREG_EINVAL;
    if (!jitter || !slots) return DREG_EINVAL;
    const RenderRecord rec = {(unsigned long long*)slots, (unsigned long long)capacity, SampleList{s_ray, s_ord, s_t, s_x, s_T_next, s_w, s_c, s_P, s_Pd}};
    return render_launch<true>(origins, viewdirs, jitter, n_rays, binary, rx, ry, rz, coarse_bits, table, w1, w2, cw1, cw2, cw3, offset, size, res, scale, hashed,
                               roi_aabb, scene_aabb, model_aabb, near_plane, far_plane, render_step_size, alpha_thre, early_stop_eps, bkgd,
                               rgb, opacity, depth, n_samples, queue, g_render_samples_waves, &rec, stream);
}

// The per-sample gradients of n records (any order) for the per-ray upstream gradients g_rgb [n_rays,3], g_opacity [n_rays], g_depth [n_rays]
// (device, fp32; each may be null = zeros; with all three null nothing is launched or written).  viewdirs, rgb, opacity, depth: the forward's
// per-ray inputs / outputs.  Writes dirs [n,3], g_sigma [n], g_c [n,3]: with the records' x, dreg_ngp_points_bwd's inputs.
int dreg_ngp_samples_grad(long n, const int* s_ray, const float* s_t, const float* s_T_next, const float* s_w, const float* s_c, const float* s_P,
                          const float* s_Pd, const float* viewdirs, const float* rgb, const float* opacity, const float* depth,
                          const float* g_rgb, const float* g_opacity, const float* g_depth, float render_step_size,
                          float* dirs, float* g_sigma, float* g_c, void* stream)
{
    if (n < 0) return DREG_EINVAL;
    if (n == 0) return DREG_OK;
    if (!s_ray || !s_t || !s_T_next || !s_w || !s_c || !s_P || !s_Pd || !viewdirs || !rgb || !opacity || !depth || !dirs || !g_sigma || !g_c)
        return DREG_EINVAL;
    if (!(render_step_size > 0.f)) return DREG_EINVAL;
    if (!g_rgb && !g_opacity && !g_depth) return DREG_OK;
    SamplesGradArgs a = {n, s_ray, s_t, s_T_next, s_w, s_c, s_P, s_Pd, viewdirs, rgb, opacity, depth, g_rgb, g_opacity, g_depth, render_step_size,
                         dirs, g_sigma, g_c};
    hipLaunchKernelGGL(ngp_samples_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

#ifdef DREG_PROBE
void dreg_render_samples_set_waves(int n) { g_render_samples_waves = n > 0 ? n : 2048; }
#endif

}  // extern "C"
