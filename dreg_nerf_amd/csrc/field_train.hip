// Training of a NeRF block's field on POINTS (gfx950): the backward of the inference forward (density phase of ngp_field.h + the per-direction
// colour net of ngp_rgb_kernel) for two given upstream gradients, dL/dsigma [n] and dL/drgb [n,3].  The rule is DESIGN.md §3m; it is §3c's
// tail ("then through the sigmoid, the colour net, ...") with the ray part replaced by the two upstream gradients.  fp64 restatement:
// tests/field_points_restatement.py.
//
// Point i, position x_i in the field's frame, unit direction d_i.  The forward is recomputed exactly (hash gather, 32 -> 64 -> 16 on the fp16
// copies, raw = fp16 h0 | 15 features; fp16 SH4(d) | 15 features | 1 -> 64 -> 64 -> 3, fp16 sigmoid), then
//   dL/dh0 = g_sigma exp(min(h0 - 1, 15))  inside the model aabb, 0 outside          dL/do_c = g_rgb_c c (1 - c)
//   d2 = relu'(h2) W3[0:3]^T do,  d1 = relu'(h1) W2^T d2,  dout = (dh0 | W1[:, 16:31]^T d1),  dh = relu'(hd) W2d^T dout,  de = W1d^T dh
//   table[corner of level l][f] += wt de[2 l + f]
// and the five weight gradients are the point sums of the outer products do x h2, d2 x h1, d1 x xin, dout x hd, dh x enc.
//
// ngp_points_bwd_kernel: one wave, 64 points per pass.  The points are cut into chunks that depend on n only (64 points each up to 131,072
// points, at most 2,048 chunks: bwd_chunk_rays' rule of render_train.hip); a wave takes the next chunk from a queue (one atomic per chunk).
// The whole chain runs on the fp32 MFMA (v_mfma_f32_16x16x4_f32) through ONE fp32 LDS tile sA [64 points][<= 64 units] that holds the current
// layer's gradient dY:
//   * the weight gradient of the layer = sum over the wave's 64 points of dY x X (X: the layer's fp16 input rows, still in LDS from the forward),
//     added into the chunk's own fp32 slab in global memory (the wave owns it: plain loads and stores);
//   * dX = dY W (W: the fp16 inference copy, widened), masked by the ReLU of the layer below, written back into sA.
// No lane holds a weight or an activation array.  The table gradient is scattered per lane (= point) with fp32 atomic adds, 16 x 8 x 2 per
// point whose dL/dh0 or colour gradient is not zero.  ngp_points_reduce_kernel then sums the slabs in chunk order: the MLP weight gradients are
// bit-identical between runs and launch widths.
#include "march.h"
#include "../../include/dreg_nerf.h"   // signature check of the entry points defined here

// one slab = the five weight matrices in parameter order (render_train.hip's layout): density W1 [64][32], W2 [16][64] (= mlp_base.params[0:3072]),
// colour W1 [64][32], W2 [64][64], W3 [16][64] (= color_mlp.params)
constexpr int PB_SLAB = 10240;
constexpr int PB_OFF_D1 = 0, PB_OFF_D2 = 2048, PB_OFF_C1 = 3072, PB_OFF_C2 = 5120, PB_OFF_C3 = 9216;
constexpr long PB_MAX_CHUNKS = 2048;
constexpr int PB_AS = 68;              // row stride (floats) of sA

struct PointsBwdArgs {
    const float *x, *dirs;
    long n;
    const _Float16 *table, *w1, *w2, *cw1, *cw2, *cw3;
    NgpLevels lv;
    float model[6];
    const float *g_sigma, *g_rgb;      // either may be null (zeros)
    float* grad_table;                 // fp32 [entries][2], accumulated with atomics
    float* slabs;                      // fp32 [n_chunks][PB_SLAB], zeroed by the entry point
    long chunk_pts;
    int n_chunks;
    unsigned int* queue;               // chunk counter, zeroed by the entry point
};

DREG_KNOB(int, g_points_bwd_waves, 2048);     // tuning (include/dreg_nerf_probe.h): one-wave workgroups of the launch; same results at every width

static long points_chunk(long n)
{
    const long waves = (n + 63) / 64;
    return 64 * ((waves + PB_MAX_CHUNKS - 1) / PB_MAX_CHUNKS);
}

// W[m][n] += sum_s sA[s][m] X(s, n) over the wave's 64 points, for the MT x NT 16x16 tiles of W (row stride ld) in the chunk's slab.  X: fp16 LDS rows.
template <int MT, int NT>
__device__ __forceinline__ void pb_outer(float* slab, int ld, const float* sA, const char* sXin, int xrs, int lane)
{
    const int fr = lane & 15, kq = lane >> 4;
#pragma unroll 1
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll 1
        for (int nt = 0; nt < NT; ++nt) {
            f32x4_t acc = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
            for (int kk = 0; kk < 16; ++kk) {
                const int s = kk * 4 + kq;
                const float xv = (float)reinterpret_cast<const _Float16*>(sXin + s * xrs)[nt * 16 + fr];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(sA[s * PB_AS + mt * 16 + fr], xv, acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) slab[(mt * 16 + kq * 4 + r) * ld + nt * 16 + fr] += acc[r];    // W[mt*16 + kq*4 + r][nt*16 + fr]
        }
}

// dX[p][c0 + i] = sum_{k < 4 KS} sA[p][k] W[k][c0 + i], i < 16 NT, for the wave's 64 points (W: fp16 [.][ld], rows = the layer's outputs).
// acc[pt][nt][r] = dX of point pt*16 + (lane >> 4)*4 + r, column c0 + nt*16 + (lane & 15).
template <int KS, int NT>
__device__ __forceinline__ void pb_back(f32x4_t (&acc)[4][NT], const float* sA, const _Float16* __restrict__ W, int ld, int c0, int lane)
{
    const int fr = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[pt][nt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int ks = 0; ks < KS; ++ks) {
        float b[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) b[nt] = (float)W[(ks * 4 + kq) * ld + c0 + nt * 16 + fr];
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) {
            const float av = sA[(pt * 16 + fr) * PB_AS + ks * 4 + kq];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[pt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[nt], acc[pt][nt], 0, 0, 0);
        }
    }
}

// acc -> sA columns 0 .. 16 NT - 1, gated by relu'(h) of the fp16 rows sHm (null: no gate)
template <int NT>
__device__ __forceinline__ void pb_store(float* sA, const f32x4_t (&acc)[4][NT], const char* sHm, int lane)
{
    const int fr = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = pt * 16 + kq * 4 + r, c = nt * 16 + fr;
                const bool on = sHm == nullptr || (float)reinterpret_cast<const _Float16*>(sHm + p * NGP_HRS)[c] > 0.f;
                sA[p * PB_AS + c] = on ? acc[pt][nt][r] : 0.f;
            }
}

__global__ __launch_bounds__(64) void ngp_points_bwd_kernel(PointsBwdArgs a)
{
    __shared__ __attribute__((aligned(16))) char sE[64 * NGP_XRS];     // the encoding (density net's input rows)
    __shared__ __attribute__((aligned(16))) char sX[64 * NGP_XRS];     // the colour net's input rows
    __shared__ __attribute__((aligned(16))) char sH[64 * NGP_HRS];     // density hidden layer
    __shared__ __attribute__((aligned(16))) char sH1[64 * NGP_HRS];    // colour hidden layers
    __shared__ __attribute__((aligned(16))) char sH2[64 * NGP_HRS];
    __shared__ __attribute__((aligned(16))) float sA[64 * PB_AS];
    __shared__ float sOut[64];
    __shared__ __attribute__((aligned(16))) float sO[64 * 4];
    const int lane = threadIdx.x;
    const int fr = lane & 15, kq = lane >> 4;

    for (;;) {
        unsigned int chunk = 0;
        if (lane == 0) chunk = atomicAdd(a.queue, 1u);
        chunk = __shfl(chunk, 0, 64);
        if (chunk >= (unsigned int)a.n_chunks) break;
        const long p0 = (long)chunk * a.chunk_pts;
        const long p1 = min(a.n, p0 + a.chunk_pts);
        float* slab = a.slabs + (size_t)chunk * PB_SLAB;

        for (long pb = p0; pb < p1; pb += 64) {
            const long p = pb + lane;
            const bool have = p < p1;
            float x[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f}, gs = 0.f, gc[3] = {0.f, 0.f, 0.f};
            if (have) {
#pragma unroll
                for (int k = 0; k < 3; ++k) { x[k] = a.x[p * 3 + k]; d[k] = a.dirs[p * 3 + k]; }
                if (a.g_sigma) gs = a.g_sigma[p];
                if (a.g_rgb) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) gc[k] = a.g_rgb[p * 3 + k];
                }
            }
            const bool live = gs != 0.f || gc[0] != 0.f || gc[1] != 0.f || gc[2] != 0.f;
            if (!__any(live)) continue;                       // nothing arrives at these 64 points: nothing is added anywhere
            // ---- the forward, sample for sample (ngp_field.h, march.h); lanes without a point take zero rows: every LDS row is written and finite
            float u[3];
            const bool inside_m = ngp_unit_cube(x, a.model, a.model + 3, 0, u) && have;
            {
                _Float16* er = reinterpret_cast<_Float16*>(sE + lane * NGP_XRS);
#pragma unroll 2
                for (int l = 0; l < 16; ++l) {
                    float f0 = 0.f, f1 = 0.f;
                    if (have) ngp_level_features(a.table, a.lv, l, u, f0, f1);
                    er[2 * l] = (_Float16)f0; er[2 * l + 1] = (_Float16)f1;
                }
                NgpDensityW dw;
                ngp_load_density_w(dw, a.w1, a.w2, lane);
                ngp_density_mlp(dw, sE, sH, lane, [&](int rb, const f32x4_t& ov) {      // ov[r] = output fr of point rb*16 + kq*4 + r
                    if (fr == 0) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) sOut[rb * 16 + kq * 4 + r] = (float)(_Float16)ov[r];
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) reinterpret_cast<_Float16*>(sX + (rb * 16 + kq * 4 + r) * NGP_XRS)[15 + fr] = (_Float16)ov[r];
                    }
                });
                uint32_t sh2[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) sh2[j] = 0u;
                if (have) render_sh4_f16(d, sh2);
                march_color_row(sX, lane, sh2);
                f16x8_t cw1f[4], cw3f[2];
                march_load_color_w(cw1f, cw3f, a.cw1, a.cw3, lane);
                march_color(sX, sH1, sH2, sO, cw1f, a.cw2, cw3f, lane);
            }
            // ---- this lane's point: dL/d(colour pre-activation) and dL/dh0
            float dO[3], dh0 = 0.f;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float c = march_sigmoid_f16(sO[lane * 4 + ch]);
                dO[ch] = gc[ch] * c * (1.f - c);
            }
            if (inside_m) dh0 = gs * __expf(fminf(sOut[lane] - 1.f, 15.f));
            float* rowA = sA + lane * PB_AS;
            // colour W3 (rows 0..2 of 16): dW3[c][i] += dO[c] h2[i];  d2 = relu'(h2) W3[0:3]^T dO (K = 4: column 3 of sA is 0)
#pragma unroll
            for (int c = 0; c < 16; ++c) rowA[c] = c < 3 ? dO[c] : 0.f;
            wave_sync();
            pb_outer<1, 4>(slab + PB_OFF_C3, 64, sA, sH2, NGP_HRS, lane);
            {
                f32x4_t acc[4][4];
                pb_back<1, 4>(acc, sA, a.cw3, 64, 0, lane);
                wave_sync();
                pb_store<4>(sA, acc, sH2, lane);
            }
            wave_sync();
            // colour W2: dW2[j][i] += d2[j] h1[i];  d1 = relu'(h1) W2^T d2
            pb_outer<4, 4>(slab + PB_OFF_C2, 64, sA, sH1, NGP_HRS, lane);
            {
                f32x4_t acc[4][4];
                pb_back<16, 4>(acc, sA, a.cw2, 64, 0, lane);
                wave_sync();
                pb_store<4>(sA, acc, sH1, lane);
            }
            wave_sync();
            // colour W1: dW1[i][k] += d1[i] xin[k]; the 15 feature inputs (columns 16..30) carry the gradient on: dout[k] = sum_i W1[i][15 + k] d1[i]
            pb_outer<4, 2>(slab + PB_OFF_C1, 32, sA, sX, NGP_XRS, lane);
            {
                f32x4_t acc[4][1];
                pb_back<16, 1>(acc, sA, a.cw1, 32, 16, lane);
                wave_sync();
                if (fr < 15) {
#pragma unroll
                    for (int pt = 0; pt < 4; ++pt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) sA[(pt * 16 + kq * 4 + r) * PB_AS + 1 + fr] = acc[pt][0][r];
                }
                rowA[0] = dh0;
            }
            wave_sync();
            // density W2: dW2[o][i] += dout[o] hd[i];  dh = relu'(hd) W2d^T dout
            pb_outer<1, 4>(slab + PB_OFF_D2, 64, sA, sH, NGP_HRS, lane);
            {
                f32x4_t acc[4][4];
                pb_back<4, 4>(acc, sA, a.w2, 64, 0, lane);
                wave_sync();
                pb_store<4>(sA, acc, sH, lane);
            }
            wave_sync();
            // density W1: dW1[i][k] += dh[i] enc[k];  de = W1d^T dh
            pb_outer<4, 2>(slab + PB_OFF_D1, 32, sA, sE, NGP_XRS, lane);
            {
                f32x4_t acc[4][2];
                pb_back<16, 2>(acc, sA, a.w1, 32, 0, lane);
                wave_sync();
                pb_store<2>(sA, acc, nullptr, lane);
            }
            wave_sync();
            // ---- hash encoding: the forward's corners again (ngp_level_corners), one fp32 atomic add per corner and feature
            if (dh0 != 0.f || dO[0] != 0.f || dO[1] != 0.f || dO[2] != 0.f) {      // (all zero: de is exactly 0, e.g. dL/dsigma alone at a point outside)
#pragma unroll 2
                for (int l = 0; l < 16; ++l) {
                    float* gl = a.grad_table + (size_t)a.lv.offset[l] * 2;
                    const float e0 = rowA[2 * l], e1 = rowA[2 * l + 1];
                    ngp_level_corners(a.lv, l, u, [&](size_t e, float wt) {
                        unsafeAtomicAdd(gl + e, wt * e0);
                        unsafeAtomicAdd(gl + e + 1, wt * e1);
                    });
                }
            }
            wave_sync();
        }
    }
}

// grad[e] += sum over chunks (in chunk order) of slab[c][e]: base = mlp_base.params[0:3072] gradient, color = color_mlp.params gradient
// (ngp_bwd_reduce_kernel of render_train.hip, which stays with its own translation unit)
__global__ void ngp_points_reduce_kernel(const float* __restrict__ slabs, int n_chunks, float* __restrict__ grad_base, float* __restrict__ grad_color)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= PB_SLAB) return;
    float s = 0.f;
    for (int c = 0; c < n_chunks; ++c) s += slabs[(size_t)c * PB_SLAB + e];
    if (e < PB_OFF_C1) grad_base[e] += s;
    else grad_color[e - PB_OFF_C1] += s;
}

static int points_layout(long n, long* chunk_pts, int* n_chunks, size_t* queue_off, size_t* total)
{
    if (n <= 0) return DREG_EINVAL;
    *chunk_pts = points_chunk(n);
    *n_chunks = (int)((n + *chunk_pts - 1) / *chunk_pts);
    *queue_off = (size_t)*n_chunks * PB_SLAB * sizeof(float);
    *total = *queue_off + 256;
    return DREG_OK;
}

extern "C" {

size_t dreg_ngp_points_bwd_workspace_bytes(long n)
{
    long cp; int nc; size_t qo, tot;
    return points_layout(n, &cp, &nc, &qo, &tot) == DREG_OK ? tot : 0;
}

int dreg_ngp_points_bwd(const float* x, const float* dirs, long n, const void* base16, const void* color16,
                        const uint32_t* offset, const uint32_t* size, const uint32_t* res, const float* scale, const uint32_t* hashed,
                        const float* model_aabb, const float* g_sigma, const float* g_rgb, float* grad_base, float* grad_color,
                        void* workspace, size_t workspace_bytes, void* stream)
{
    if (n < 0) return DREG_EINVAL;
    if (n == 0) return DREG_OK;
    if (!x || !dirs || !base16 || !color16 || !offset || !size || !res || !scale || !hashed || !model_aabb || !grad_base || !grad_color || !workspace)
        return DREG_EINVAL;
    for (int k = 0; k < 3; ++k)
        if (!(model_aabb[3 + k] > model_aabb[k])) return DREG_EINVAL;
    PointsBwdArgs a;
    size_t queue_off, total;
    if (points_layout(n, &a.chunk_pts, &a.n_chunks, &queue_off, &total) != DREG_OK || workspace_bytes < total) return DREG_EINVAL;
    if (!g_sigma && !g_rgb) return DREG_OK;          // both upstream gradients are zero: nothing is added
    char* ws = (char*)workspace;
    const _Float16* b16 = (const _Float16*)base16;
    const _Float16* c16 = (const _Float16*)color16;
    a.x = x; a.dirs = dirs; a.n = n;
    a.table = b16 + 3072; a.w1 = b16; a.w2 = b16 + 2048;
    a.cw1 = c16; a.cw2 = c16 + 2048; a.cw3 = c16 + 6144;
    ngp_fill_levels(a.lv, offset, size, res, scale, hashed);
    for (int k = 0; k < 6; ++k) a.model[k] = model_aabb[k];
    a.g_sigma = g_sigma; a.g_rgb = g_rgb;
    a.grad_table = grad_base + 3072;
    a.slabs = (float*)ws;
    a.queue = (unsigned int*)(ws + queue_off);
    if (hipMemsetAsync(ws, 0, total, (hipStream_t)stream) != hipSuccess) return DREG_ELAUNCH;
    long waves = a.n_chunks;
    if (waves > g_points_bwd_waves) waves = g_points_bwd_waves;
    hipLaunchKernelGGL(ngp_points_bwd_kernel, dim3((unsigned)waves), dim3(64), 0, (hipStream_t)stream, a);
    DREG_LAUNCH_CHECK();
    hipLaunchKernelGGL(ngp_points_reduce_kernel, dim3(PB_SLAB / 256), dim3(256), 0, (hipStream_t)stream, (const float*)ws, a.n_chunks, grad_base, grad_color);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

#ifdef DREG_PROBE
void dreg_points_bwd_set_waves(int n) { g_points_bwd_waves = n > 0 ? n : 2048; }
#endif

}  // extern "C"
