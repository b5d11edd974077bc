// Training of one NeRF block (Instant-NGP field + occupancy grid), gfx950: the backward of the volume renderer (render.hip) down to the hash
// table, and the fused Adam step of the field.  The rule is the reference's training step (train_ngp_nerf.py:268-335 over nerfacc 0.3.5
// ray_marching(stratified=True) + rendering), stated in DESIGN.md §3c; CPU restatement: tests/render_train_restatement.py.
//
// Backward of one ray, C its forward rgb (background included), g = dL/dC, survivors k with transmittance T_k, alpha_k, colour c_k, w_k = T_k alpha_k:
//   dL/dc_k     = w_k g
//   dL/dsigma_k = dt g . (T_{k+1} c_k - S_k),   S_k = C - sum_{j<=k} w_j c_j   (one forward sweep from the saved C)
//   dL/dh0      = dL/dsigma exp(min(h0 - 1, 15))                  (trunc_exp; 0 outside the model aabb, where sigma = 0)
// then through the sigmoid, the colour net (3 of its 16 outputs) into its 15 feature inputs, the density net, and the 16-level hash encoding
// (trilinear corner weights) into the table.  Marched samples that do not survive get no gradient.
//
// ngp_render_bwd_kernel: one lane per ray.  The rays are cut into chunks that depend on n_rays only (64 rays each up to 131,072 rays); a wave takes
// the next chunk from a queue and re-marches its rays with the forward's own helpers (march.h), so survivors and colours are those of the forward
// bit for bit.  Per pass the wave's 64 samples go through the backward together:
//   * per lane, fp32 on the VALU: the matrix-vector products of the chain (weights: fp32 copies of the fp16 inference copies, lane-uniform);
//   * per wave, on MFMA (v_mfma_f32_16x16x4_f32, fp32): the weight gradients as sample-sum outer products (K = the wave's 64 samples), added into
//     the chunk's own fp32 slab in global memory (the wave owns it: plain loads and stores);
//   * per lane: the hash-table gradient, 16 levels x 8 corners x 2 fp32 global atomic adds (order free).
// fb_reduce then sums the slabs in chunk order: the MLP weight gradients are bit-identical across runs and launch widths.  The slab layout, the
// chunk rule, the outer product (fb_outer) and the reduce are ngp_field_bwd.h's, shared with the point backward (field_train.hip).
#include "ngp_field_bwd.h"
#include "../../include/dreg_nerf.h"   // signature check of the entry points defined here

struct RenderBwdArgs : MarchBlock {    // the forward's block (march.h), then the launch's own
    const float *origins, *dirs, *jitter;
    long n_rays;
    const float* wf;                   // fp32 copies of the five weight matrices, slab layout
    float eps;
    long pass_bound;                   // passes per chunk: chunk_rays * (n_max + 2) + 64 (march_pass_bound)
    const float *rgb, *grad_rgb;       // forward rgb (with background) and dL/drgb, fp32 [N,3]
    float* grad_table;                 // fp32 [entries][2], accumulated with atomics
    float* slabs;                      // fp32 [n_chunks][FB_SLAB], zeroed by the entry point
    long chunk_rays;
    int n_chunks;
    unsigned int* queue;               // chunk counter, zeroed by the entry point
};

constexpr size_t BWD_LEAD = (size_t)FB_SLAB * sizeof(float);      // the workspace begins with wf

DREG_KNOB(int, g_render_bwd_waves, 2048);     // tuning (include/dreg_nerf_probe.h): one-wave workgroups of the backward launch; same results at every width

// the weight gradient of a layer over the surviving samples, the tile loops unrolled in full
template <int MT, int NT>
__device__ __forceinline__ void bwd_outer(float* slab, int ld, const float* sA, const char* sXin, int xrs, const float* sLive, int lane)
{
    fb_outer<MT, NT, true, true>(slab, ld, sA, sXin, xrs, sLive, lane);
}

__global__ __launch_bounds__(64) void ngp_render_bwd_kernel(RenderBwdArgs a)
{
    __shared__ __attribute__((aligned(16))) char sX[64 * NGP_XRS];     // density input, then the colour input rows, then the encoding again
    __shared__ __attribute__((aligned(16))) char sH[64 * NGP_HRS];     // density hidden layer
    __shared__ __attribute__((aligned(16))) char sH1[64 * NGP_HRS];    // colour hidden layers
    __shared__ __attribute__((aligned(16))) char sH2[64 * NGP_HRS];
    __shared__ __attribute__((aligned(16))) float sA[64 * FB_AS];
    __shared__ float sOut[64], sLive[64];
    __shared__ __attribute__((aligned(16))) float sO[64 * 4];
    __shared__ uint32_t sCoarse[1024];
    const int lane = threadIdx.x;
    march_load_coarse(sCoarse, a, lane);
    __syncthreads();
    MarchGrid g;               // march_grid's body, kept local: through the helper this kernel, at its register limit, reserved 16 more bytes of scratch per lane
    g.binary = a.binary; g.sCoarse = a.coarse != nullptr ? sCoarse : nullptr;
#pragma unroll
    for (int k = 0; k < 3; ++k) { g.roi[k] = a.roi[k]; g.roi[3 + k] = a.roi[3 + k]; g.roi_ext[k] = a.roi[3 + k] - a.roi[k]; }
    g.rdim[0] = a.rx; g.rdim[1] = a.ry; g.rdim[2] = a.rz; g.ry = a.ry; g.rz = a.rz; g.cy = a.cy; g.cz = a.cz;
    NgpDensityW dw;
    ngp_load_density_w(dw, a.w1, a.w2, lane);
    f16x8_t cw1f[4], cw3f[2];
    march_load_color_w(cw1f, cw3f, a.cw1, a.cw3, lane);
    const float* wd1 = a.wf + FB_OFF_D1;
    const float* wd2 = a.wf + FB_OFF_D2;
    const float* wc1 = a.wf + FB_OFF_C1;
    const float* wc2 = a.wf + FB_OFF_C2;
    const float* wc3 = a.wf + FB_OFF_C3;

    for (;;) {
        const unsigned int chunk = fb_next_chunk(a.queue, lane);
        if (chunk >= (unsigned int)a.n_chunks) break;
        const long r0 = (long)chunk * a.chunk_rays;
        const long r1 = min(a.n_rays, r0 + a.chunk_rays);
        float* slab = a.slabs + (size_t)chunk * FB_SLAB;
        MarchChunk own = {r0};
        bool active = false, exhausted = false;
        long ray = 0;
        int n = 0, n_lim = 0;
        float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f}, tmin = 0.f, tmax = 0.f;
        float T_all = 1.f, T_s = 1.f, acc[3] = {0.f, 0.f, 0.f}, C[3] = {0.f, 0.f, 0.f}, gr[3] = {0.f, 0.f, 0.f};
        uint32_t sh2[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) sh2[j] = 0u;

        for (long it = 0; it < a.pass_bound; ++it) {
            // ---- refill from the chunk's rays in lane order (no atomics: the chunk is this wave's)
            for (int tries = 0; tries < 1024; ++tries) {
                const bool need = !active && !exhausted;
                unsigned long long r = 0;
                if (!march_take(own, need, lane, r)) break;
                if (need) {
                    if ((long)r >= r1) exhausted = true;
                    else {
                        ray = (long)r;
#pragma unroll
                        for (int k = 0; k < 3; ++k) { o[k] = a.origins[ray * 3 + k]; d[k] = a.dirs[ray * 3 + k]; }
                        const bool hit = render_ray_interval(o, d, a.scene, a.near, a.far, tmin, tmax);
                        tmin += a.jitter[ray] * a.dt;
                        if (hit && tmin < tmax) {
                            active = true; n = 0; T_all = 1.f; T_s = 1.f;
                            n_lim = (int)fminf(ceilf((tmax - tmin) / a.dt) + 1.f, (float)a.n_max);
#pragma unroll
                            for (int k = 0; k < 3; ++k) { acc[k] = 0.f; C[k] = a.rgb[ray * 3 + k]; gr[k] = a.grad_rgb[ray * 3 + k]; }
                            render_sh4_f16(d, sh2);
                        }
                    }
                }
            }
            if (!__any(active)) {
                if (__all(exhausted)) break;
                continue;
            }
            // ---- the forward's march and density (march.h), sample for sample
            float x[3] = {0.f, 0.f, 0.f}, tm = 0.f;
            if (active && n >= n_lim) active = false;
            const bool have = march_advance(g, o, d, tmin, tmax, a.dt, n, active, x, &tm, 4096);
            if (!__any(have)) continue;
            const bool inside_m = march_density<true>(have, x, a.model, a.lv, a.table, dw, sX, sH, sOut, lane);
            bool surv = false;
            float w = 0.f, h0 = 0.f;
            if (have) {
                h0 = sOut[lane];
                surv = march_composite(march_sigma(inside_m, h0), 1.f, a.dt, a.eps, a.alpha_thre, T_all, T_s, w);      // (a survivor's T_s is now T_{k+1})
                ++n;
                if (surv) march_color_row(sX, lane, sh2);
            }
            if (__any(surv)) {
                sLive[lane] = surv ? 1.f : 0.f;
                march_color(sX, sH1, sH2, sO, cw1f, a.cw2, cw3f, lane);
                // ---- this lane's survivor: dL/d(colour pre-activation) and dL/dh0
                float dO[3] = {0.f, 0.f, 0.f}, dh0 = 0.f;
                if (surv) {
                    float dsig = 0.f;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const float c = march_sigmoid_f16(sO[lane * 4 + ch]);
                        acc[ch] += w * c;
                        dsig += gr[ch] * (T_s * c - (C[ch] - acc[ch]));
                        dO[ch] = w * gr[ch] * c * (1.f - c);
                    }
                    dh0 = inside_m ? a.dt * dsig * __expf(fminf(h0 - 1.f, 15.f)) : 0.f;
                }
                float* rowA = sA + lane * FB_AS;
                // colour W3 (rows 0..2 of 16): dW3[c][i] += dO[c] h2[i]
#pragma unroll
                for (int c = 0; c < 16; ++c) rowA[c] = c < 3 ? dO[c] : 0.f;
                wave_sync();
                bwd_outer<1, 4>(slab + FB_OFF_C3, 64, sA, sH2, NGP_HRS, sLive, lane);
                const _Float16* h2 = reinterpret_cast<const _Float16*>(sH2 + lane * NGP_HRS);
                const _Float16* h1 = reinterpret_cast<const _Float16*>(sH1 + lane * NGP_HRS);
                float d2[64];
#pragma unroll
                for (int i = 0; i < 64; ++i) {
                    const float s = wc3[i] * dO[0] + wc3[64 + i] * dO[1] + wc3[128 + i] * dO[2];
                    d2[i] = (float)h2[i] > 0.f ? s : 0.f;
                }
                wave_sync();
                // colour W2: dW2[j][i] += d2[j] h1[i]
#pragma unroll
                for (int j = 0; j < 64; ++j) rowA[j] = d2[j];
                wave_sync();
                bwd_outer<4, 4>(slab + FB_OFF_C2, 64, sA, sH1, NGP_HRS, sLive, lane);
                float d1[64];
#pragma unroll
                for (int i = 0; i < 64; ++i) d1[i] = 0.f;
#pragma unroll
                for (int j = 0; j < 64; ++j) {
                    const float dj = d2[j];
#pragma unroll
                    for (int i = 0; i < 64; ++i) d1[i] += wc2[j * 64 + i] * dj;
                }
#pragma unroll
                for (int i = 0; i < 64; ++i) d1[i] = (float)h1[i] > 0.f ? d1[i] : 0.f;
                wave_sync();
                // colour W1: dW1[i][k] += d1[i] x[k]; the 15 feature inputs (columns 16..30) carry the gradient on
#pragma unroll
                for (int i = 0; i < 64; ++i) rowA[i] = d1[i];
                wave_sync();
                bwd_outer<4, 2>(slab + FB_OFF_C1, 32, sA, sX, NGP_XRS, sLive, lane);
                float dout[16];
                dout[0] = dh0;
#pragma unroll
                for (int k = 1; k < 16; ++k) dout[k] = 0.f;
#pragma unroll
                for (int i = 0; i < 64; ++i) {
                    const float di = d1[i];
#pragma unroll
                    for (int k = 1; k < 16; ++k) dout[k] += wc1[i * 32 + 15 + k] * di;
                }
                wave_sync();
                // density W2: dW2[o][i] += dout[o] hd[i]
#pragma unroll
                for (int k = 0; k < 16; ++k) rowA[k] = dout[k];
                wave_sync();
                bwd_outer<1, 4>(slab + FB_OFF_D2, 64, sA, sH, NGP_HRS, sLive, lane);
                const _Float16* hd = reinterpret_cast<const _Float16*>(sH + lane * NGP_HRS);
                float dh[64];
#pragma unroll
                for (int i = 0; i < 64; ++i) {
                    float s = 0.f;
#pragma unroll
                    for (int k = 0; k < 16; ++k) s += wd2[k * 64 + i] * dout[k];
                    dh[i] = (float)hd[i] > 0.f ? s : 0.f;
                }
                float de[32];
#pragma unroll
                for (int k = 0; k < 32; ++k) de[k] = 0.f;
#pragma unroll
                for (int i = 0; i < 64; ++i) {
                    const float di = dh[i];
#pragma unroll
                    for (int k = 0; k < 32; ++k) de[k] += wd1[i * 32 + k] * di;
                }
                wave_sync();
#pragma unroll
                for (int i = 0; i < 64; ++i) rowA[i] = dh[i];
                // ---- hash encoding: the forward's corners again (ngp_level_corners of ngp_field.h, as march_density); the encoding goes back into
                // sX for dW1 of the density net, the gradient into the table with one fp32 atomic add per corner and feature
                if (surv) {
                    float u[3];
                    (void)ngp_unit_cube(x, a.model, a.model + 3, 0, u);
                    _Float16* xr = reinterpret_cast<_Float16*>(sX + lane * NGP_XRS);
#pragma unroll 2
                    for (int l = 0; l < 16; ++l) {
                        const _Float16* tl = a.table + (size_t)a.lv.offset[l] * 2;
                        float* gl = a.grad_table + (size_t)a.lv.offset[l] * 2;
                        float f0 = 0.f, f1 = 0.f;
                        const float e0 = de[2 * l], e1 = de[2 * l + 1];
                        ngp_level_corners(a.lv, l, u, [&](size_t e, float wt) {
                            ngp_corner_accumulate(tl, e, wt, f0, f1);
                            unsafeAtomicAdd(gl + e, wt * e0);
                            unsafeAtomicAdd(gl + e + 1, wt * e1);
                        });
                        xr[2 * l] = (_Float16)f0; xr[2 * l + 1] = (_Float16)f1;
                    }
                }
                wave_sync();
                // density W1: dW1[i][k] += dh[i] enc[k]
                bwd_outer<4, 2>(slab + FB_OFF_D1, 32, sA, sX, NGP_XRS, sLive, lane);
            }
            if (have && T_all < a.eps) active = false;           // transmittance below early_stop_eps: the ray ends
            wave_sync();
        }
    }
}

// fp32 copies of the five weight matrices in slab layout, from the fp16 inference copies
__global__ void ngp_bwd_weights_kernel(const _Float16* __restrict__ base16, const _Float16* __restrict__ col16, float* __restrict__ wf)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= FB_SLAB) return;
    wf[e] = e < FB_OFF_C1 ? (float)base16[e] : (float)col16[e - FB_OFF_C1];
}

// torch.optim.Adam (single-tensor arithmetic, no weight decay) + the fp16 inference copy + a zeroed gradient, in one pass
__global__ void ngp_adam_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, _Float16* __restrict__ p16,
                                size_t n, float lr, float beta1, float beta2, float eps, float step_size, float bc2_sqrt)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float gi = g[i];
        float mi = m[i], vi = v[i];
        mi = mi + (1.f - beta1) * (gi - mi);                          // exp_avg.lerp_(grad, 1 - beta1)
        vi = vi * beta2 + (1.f - beta2) * (gi * gi);                  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
        const float denom = __builtin_sqrtf(vi) / bc2_sqrt + eps;
        const float pi = p[i] - step_size * (mi / denom);             // param.addcdiv_(exp_avg, denom, value=-step_size)
        m[i] = mi; v[i] = vi; p[i] = pi;
        p16[i] = (_Float16)pi;
        g[i] = 0.f;
    }
}

extern "C" {

size_t dreg_ngp_render_bwd_workspace_bytes(long n_rays)
{
    FbLayout w;
    return fb_layout(n_rays, BWD_LEAD, w) == DREG_OK ? w.total : 0;
}

int dreg_ngp_render_bwd(const float* origins, const float* viewdirs, const float* jitter, long n_rays, const uint8_t* binary, int rx, int ry, int rz,
                        const uint32_t* coarse_bits, const void* base16, const void* color16,
                        const uint32_t* offset, const uint32_t* size, const uint32_t* res, const float* scale, const uint32_t* hashed,
                        const float* roi_aabb, const float* scene_aabb, const float* model_aabb, float near_plane, float far_plane,
                        float render_step_size, float alpha_thre, float early_stop_eps,
                        const float* rgb, const float* grad_rgb, float* grad_base, float* grad_color, void* workspace, size_t workspace_bytes, void* stream)
{
    if (n_rays < 0) return DREG_EINVAL;
    if (n_rays == 0) return DREG_OK;
    if (!origins || !viewdirs || !jitter || !base16 || !color16 || !rgb || !grad_rgb || !grad_base || !grad_color || !workspace) return DREG_EINVAL;
    RenderBwdArgs a;
    FbLayout w;
    if (fb_layout(n_rays, BWD_LEAD, w) != DREG_OK || workspace_bytes < w.total) return DREG_EINVAL;
    a.chunk_rays = w.chunk_items; a.n_chunks = w.n_chunks;
    char* ws = (char*)workspace;
    a.origins = origins; a.dirs = viewdirs; a.jitter = jitter; a.n_rays = n_rays;
    const NgpParams16 p = ngp_split_params(base16, color16);
    if (march_fill_block(a, binary, rx, ry, rz, coarse_bits, p.table, p.w1, p.w2, true, p.cw1, p.cw2, p.cw3, offset, size, res, scale, hashed,
                         roi_aabb, scene_aabb, model_aabb, near_plane, far_plane, render_step_size, alpha_thre, true) != DREG_OK)
        return DREG_EINVAL;
    a.wf = (const float*)ws;
    a.eps = early_stop_eps;
    a.pass_bound = march_pass_bound(a.chunk_rays, (double)(a.n_max + 2));
    a.rgb = rgb; a.grad_rgb = grad_rgb;
    a.grad_table = grad_base + NGP_BASE_TABLE;
    a.slabs = (float*)(ws + w.slab_off);
    a.queue = (unsigned int*)(ws + w.queue_off);
    if (hipMemsetAsync(ws + w.slab_off, 0, w.total - w.slab_off, (hipStream_t)stream) != hipSuccess) return DREG_ELAUNCH;
    hipLaunchKernelGGL(ngp_bwd_weights_kernel, dim3(FB_SLAB / 256), dim3(256), 0, (hipStream_t)stream, (const _Float16*)base16, (const _Float16*)color16,
                       (float*)ws);
    DREG_LAUNCH_CHECK();
    long waves = a.n_chunks;
    if (waves > g_render_bwd_waves) waves = g_render_bwd_waves;
    hipLaunchKernelGGL(ngp_render_bwd_kernel, dim3((unsigned)waves), dim3(64), 0, (hipStream_t)stream, a);
    DREG_LAUNCH_CHECK();
    return fb_reduce(a.slabs, a.n_chunks, grad_base, grad_color, (hipStream_t)stream);
}

int dreg_ngp_adam_step(float* p, float* g, float* m, float* v, void* p16, size_t n, float lr, float beta1, float beta2, float eps, int step, void* stream)
{
    if (n == 0) return DREG_OK;
    if (!p || !g || !m || !v || !p16 || step < 1) return DREG_EINVAL;
    const double bc1 = 1.0 - __builtin_pow((double)beta1, (double)step), bc2 = 1.0 - __builtin_pow((double)beta2, (double)step);
    size_t b = (n + 255) / 256; if (b > 8192) b = 8192;
    hipLaunchKernelGGL(ngp_adam_kernel, dim3((unsigned)b), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (_Float16*)p16, n, lr, beta1, beta2, eps,
                       (float)(lr / bc1), (float)__builtin_sqrt(bc2));
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

#ifdef DREG_PROBE
void dreg_render_bwd_set_waves(int n) { g_render_bwd_waves = n > 0 ? n : 2048; }
#endif

}  // extern "C"
