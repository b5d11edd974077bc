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
// ngp_points_bwd_kernel: one wave, 64 points per pass.  The points are cut into chunks that depend on n only (fb_layout of ngp_field_bwd.h, the
// render backward's rule); a wave takes the next chunk from a queue (one atomic per chunk).  The forward is field_point_forward; the whole chain
// then runs on the fp32 MFMA (v_mfma_f32_16x16x4_f32) through ONE fp32 LDS tile sA [64 points][<= 64 units] that holds the current layer's
// gradient dY, with the functions of ngp_field_bwd.h:
//   * fb_outer: the weight gradient of the layer = sum over the wave's 64 points of dY x X (X: the layer's fp16 input rows, still in LDS from the
//     forward), added into the chunk's own fp32 slab in global memory (the wave owns it: plain loads and stores);
//   * fb_back, fb_store: dX = dY W (W: the fp16 inference copy, widened), masked by the ReLU of the layer below, written back into sA.
// No lane holds a weight or an activation array.  The table gradient is scattered per lane (= point) with fp32 atomic adds, 16 x 8 x 2 per
// point whose dL/dh0 or colour gradient is not zero.  fb_reduce then sums the slabs in chunk order: the MLP weight gradients are bit-identical
// between runs and launch widths.
#include "ngp_field_bwd.h"
#include "../../include/dreg_nerf.h"   // signature check of the entry points defined here

struct PointsBwdArgs : FieldPointArgs {
    float* grad_table;                 // fp32 [entries][2], accumulated with atomics
    float* slabs;                      // fp32 [n_chunks][FB_SLAB], zeroed by the entry point
    long chunk_pts;
    int n_chunks;
    unsigned int* queue;               // chunk counter, zeroed by the entry point
};

DREG_KNOB(int, g_points_bwd_waves, 2048);     // tuning (include/dreg_nerf_probe.h): one-wave workgroups of the launch; same results at every width

// the weight gradient of a layer over all 64 points, the tile loops kept as loops
template <int MT, int NT>
__device__ __forceinline__ void pb_outer(float* slab, int ld, const float* sA, const char* sXin, int xrs, int lane)
{
    fb_outer<MT, NT, false, false>(slab, ld, sA, sXin, xrs, nullptr, lane);
}

__global__ __launch_bounds__(64) void ngp_points_bwd_kernel(PointsBwdArgs a)
{
    __shared__ __attribute__((aligned(16))) char sE[64 * NGP_XRS];     // the encoding (density net's input rows)
    __shared__ __attribute__((aligned(16))) char sX[64 * NGP_XRS];     // the colour net's input rows
    __shared__ __attribute__((aligned(16))) char sH[64 * NGP_HRS];     // density hidden layer
    __shared__ __attribute__((aligned(16))) char sH1[64 * NGP_HRS];    // colour hidden layers
    __shared__ __attribute__((aligned(16))) char sH2[64 * NGP_HRS];
    __shared__ __attribute__((aligned(16))) float sA[64 * FB_AS];
    __shared__ float sOut[64];
    __shared__ __attribute__((aligned(16))) float sO[64 * 4];
    const int lane = threadIdx.x;
    const int fr = lane & 15, kq = lane >> 4;

    for (;;) {
        const unsigned int chunk = fb_next_chunk(a.queue, lane);
        if (chunk >= (unsigned int)a.n_chunks) break;
        const long p0 = (long)chunk * a.chunk_pts;
        const long p1 = min(a.n, p0 + a.chunk_pts);
        float* slab = a.slabs + (size_t)chunk * FB_SLAB;

        for (long pb = p0; pb < p1; pb += 64) {
            // ---- the forward, sample for sample; false: nothing arrives at these 64 points, nothing is added anywhere
            FieldPoint fp;
            if (!field_point_forward(a, pb + lane, pb + lane < p1, sE, sH, sX, sH1, sH2, sOut, sO, lane, fp, [] {})) continue;
            const float (&dO)[3] = fp.dO;
            const float dh0 = fp.dh0;
            float* rowA = sA + lane * FB_AS;
            // colour W3 (rows 0..2 of 16): dW3[c][i] += dO[c] h2[i];  d2 = relu'(h2) W3[0:3]^T dO (K = 4: column 3 of sA is 0)
#pragma unroll
            for (int c = 0; c < 16; ++c) rowA[c] = c < 3 ? dO[c] : 0.f;
            wave_sync();
            pb_outer<1, 4>(slab + FB_OFF_C3, 64, sA, sH2, NGP_HRS, lane);
            {
                f32x4_t acc[4][4];
                fb_back<1, 4>(acc, sA, a.cw3, 64, 0, lane);
                wave_sync();
                fb_store<4>(sA, acc, FbGateLds{sH2}, lane);
            }
            wave_sync();
            // colour W2: dW2[j][i] += d2[j] h1[i];  d1 = relu'(h1) W2^T d2
            pb_outer<4, 4>(slab + FB_OFF_C2, 64, sA, sH1, NGP_HRS, lane);
            {
                f32x4_t acc[4][4];
                fb_back<16, 4>(acc, sA, a.cw2, 64, 0, lane);
                wave_sync();
                fb_store<4>(sA, acc, FbGateLds{sH1}, lane);
            }
            wave_sync();
            // colour W1: dW1[i][k] += d1[i] xin[k]; the 15 feature inputs (columns 16..30) carry the gradient on: dout[k] = sum_i W1[i][15 + k] d1[i]
            pb_outer<4, 2>(slab + FB_OFF_C1, 32, sA, sX, NGP_XRS, lane);
            {
                f32x4_t acc[4][1];
                fb_back<16, 1>(acc, sA, a.cw1, 32, 16, lane);
                wave_sync();
                if (fr < 15) {
#pragma unroll
                    for (int pt = 0; pt < 4; ++pt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) sA[(pt * 16 + kq * 4 + r) * FB_AS + 1 + fr] = acc[pt][0][r];
                }
                rowA[0] = dh0;
            }
            wave_sync();
            // density W2: dW2[o][i] += dout[o] hd[i];  dh = relu'(hd) W2d^T dout
            pb_outer<1, 4>(slab + FB_OFF_D2, 64, sA, sH, NGP_HRS, lane);
            {
                f32x4_t acc[4][4];
                fb_back<4, 4>(acc, sA, a.w2, 64, 0, lane);
                wave_sync();
                fb_store<4>(sA, acc, FbGateLds{sH}, lane);
            }
            wave_sync();
            // density W1: dW1[i][k] += dh[i] enc[k];  de = W1d^T dh
            pb_outer<4, 2>(slab + FB_OFF_D1, 32, sA, sE, NGP_XRS, lane);
            {
                f32x4_t acc[4][2];
                fb_back<16, 2>(acc, sA, a.w1, 32, 0, lane);
                wave_sync();
                fb_store<2>(sA, acc, FbGateNone{}, lane);
            }
            wave_sync();
            // ---- hash encoding: the forward's corners again (ngp_level_corners), one fp32 atomic add per corner and feature
            if (dh0 != 0.f || dO[0] != 0.f || dO[1] != 0.f || dO[2] != 0.f) {      // (all zero: de is exactly 0, e.g. dL/dsigma alone at a point outside)
#pragma unroll 2
                for (int l = 0; l < 16; ++l) {
                    float* gl = a.grad_table + (size_t)a.lv.offset[l] * 2;
                    const float e0 = rowA[2 * l], e1 = rowA[2 * l + 1];
                    ngp_level_corners(a.lv, l, fp.u, [&](size_t e, float wt) {
                        unsafeAtomicAdd(gl + e, wt * e0);
                        unsafeAtomicAdd(gl + e + 1, wt * e1);
                    });
                }
            }
            wave_sync();
        }
    }
}

// fb_reduce of ngp_field_bwd.h, defined here for the library (render_train.hip calls it too)
__global__ void fb_reduce_kernel(const float* __restrict__ slabs, int n_chunks, float* __restrict__ grad_base, float* __restrict__ grad_color)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= FB_SLAB) return;
    float s = 0.f;
    for (int c = 0; c < n_chunks; ++c) s += slabs[(size_t)c * FB_SLAB + e];
    if (e < FB_OFF_C1) grad_base[e] += s;
    else grad_color[e - FB_OFF_C1] += s;
}
int fb_reduce(const float* slabs, int n_chunks, float* grad_base, float* grad_color, hipStream_t stream)
{
    hipLaunchKernelGGL(fb_reduce_kernel, dim3(FB_SLAB / 256), dim3(256), 0, stream, slabs, n_chunks, grad_base, grad_color);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

extern "C" {

size_t dreg_ngp_points_bwd_workspace_bytes(long n)
{
    FbLayout w;
    return fb_layout(n, 0, w) == DREG_OK ? w.total : 0;
}

int dreg_ngp_points_bwd(const float* x, const float* dirs, long n, const void* base16, const void* color16,
                        const uint32_t* offset, const uint32_t* size, const uint32_t* res, const float* scale, const uint32_t* hashed,
                        const float* model_aabb, const float* g_sigma, const float* g_rgb, float* grad_base, float* grad_color,
                        void* workspace, size_t workspace_bytes, void* stream)
{
    if (n < 0) return DREG_EINVAL;
    if (n == 0) return DREG_OK;
    if (!grad_base || !grad_color || !workspace) return DREG_EINVAL;
    PointsBwdArgs a;
    if (field_fill_points(a, x, dirs, n, base16, color16, offset, size, res, scale, hashed, model_aabb, g_sigma, g_rgb) != DREG_OK) return DREG_EINVAL;
    FbLayout w;
    if (fb_layout(n, 0, w) != DREG_OK || workspace_bytes < w.total) return DREG_EINVAL;
    if (!g_sigma && !g_rgb) return DREG_OK;          // both upstream gradients are zero: nothing is added
    char* ws = (char*)workspace;
    a.grad_table = grad_base + NGP_BASE_TABLE;
    a.slabs = (float*)(ws + w.slab_off);
    a.chunk_pts = w.chunk_items; a.n_chunks = w.n_chunks;
    a.queue = (unsigned int*)(ws + w.queue_off);
    if (hipMemsetAsync(ws, 0, w.total, (hipStream_t)stream) != hipSuccess) return DREG_ELAUNCH;
    long waves = a.n_chunks;
    if (waves > g_points_bwd_waves) waves = g_points_bwd_waves;
    hipLaunchKernelGGL(ngp_points_bwd_kernel, dim3((unsigned)waves), dim3(64), 0, (hipStream_t)stream, a);
    DREG_LAUNCH_CHECK();
    return fb_reduce(a.slabs, a.n_chunks, grad_base, grad_color, (hipStream_t)stream);
}

#ifdef DREG_PROBE
void dreg_points_bwd_set_waves(int n) { g_points_bwd_waves = n > 0 ? n : 2048; }
#endif

}  // extern "C"
