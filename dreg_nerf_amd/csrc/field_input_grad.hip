// Input gradients of a NeRF block's field (gfx950): dL/dx and dL/ddir at POINTS for two given upstream gradients, dL/dsigma [n] and dL/drgb [n,3],
// with the parameters frozen, and their sums along rays.  The rule is DESIGN.md §3p; fp64 restatement: tests/field_input_grad_restatement.py.
//
// Point i, position x_i in the field's frame, direction d_i (used as given).  The forward is ngp_points_bwd_kernel's (field_train.hip): both
// call field_point_forward of ngp_field_bwd.h; and the chain is that kernel's (fb_back, fb_store), the fp16 roundings taken as identity:
//   dL/dh0 = g_sigma exp(min(h0 - 1, 15))  inside the model aabb, 0 outside          dL/do_c = g_rgb_c c (1 - c)
//   d2 = relu'(h2) W3[0:3]^T do,  d1 = relu'(h1) W2^T d2,  dsh = W1[:, 0:16]^T d1,  dout = (dh0 | W1[:, 16:31]^T d1),
//   dh = relu'(hd) W2d^T dout,  de = W1d^T dh
// with two tails, one lane per point:
//   dL/dd_c = sum_j dsh[j] dsh4_j/dd_c                         (the degree-4 polynomials of render_sh4_f16, differentiated in fp32)
//   du_c = sum_l scale_l sum_corners (+-1)(w_a w_b)(de[2l] t_0 + de[2l+1] t_1),   dL/dx_c = du_c / (hi_c - lo_c) where 0 < u_c < 1, else exactly 0
// (ngp_encoding_dx of ngp_field.h, which ngp_grad.hip calls too).  The colour term does not depend on the aabb: a point outside on one axis
// keeps it on the other two.
//
// ngp_points_input_grad_kernel: one wave, 64 points per pass.  Nothing here needs an activation, only the three ReLU gates: each lane takes its
// point's gates as 64-bit masks during the forward (ngp_relu_mask of ngp_field.h, as ngp_grad.hip does), so the forward's tiles are dead when
// the chain starts and the chain's fp32 tile sA [64 points][<= 64 units] lies over them.  LDS: two hidden tiles of 9,216 B (the encoding
// aliases the head of the first, the colour net's input rows the head of the second, which is also the colour net's second hidden tile) +
// 1,280 B of outputs = 19,712 B.  A gate of another lane's point is fetched with a shuffle when the gated tile is stored (FbGateMask).  No
// weight gradients: no slabs, no atomics, no reduce pass, no workspace.
//
// ngp_samples_ray_grad_kernel: one lane per ray.  The list is in canonical order (ascending ray, then ord), so a ray's records are one
// contiguous segment; the lane finds its start by bisection on the ray column and adds the segment in order: deterministic by construction.
#include "ngp_field_bwd.h"
#include "../../include/dreg_nerf.h"   // signature check of the entry points defined here

constexpr int IG_TILE = 64 * NGP_HRS;  // one hidden tile

struct InputGradArgs : FieldPointArgs {
    float *grad_x, *grad_dir;          // either may be null (not written)
};

// dL/dd_c = sum_j g[j] dsh4_j/dd_c: the polynomials of render_sh4_f16 differentiated term by term (g[0] meets the constant)
__device__ __forceinline__ void ig_sh4_grad(const float (&d)[3], const float* g, float (&out)[3])
{
    const float x = d[0], y = d[1], z = d[2];
    const float xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
    constexpr float C1 = 0.48860251190291987f, C2 = 1.0925484305920792f, C3 = 0.94617469575755997f, C4 = 0.54627421529603959f,
                    C5 = 0.59004358992664352f, C6 = 2.8906114426405538f, C7 = 0.45704579946446572f, C8 = 0.3731763325901154f, C9 = 1.4453057213202769f;
    const float q = 1.0f - 5.0f * z2, s = 3.0f * (y2 - x2);
    out[0] = -C1 * g[3] + C2 * (y * g[4] - z * g[7]) + 2.0f * C4 * x * g[8] - 6.0f * C5 * xy * g[9] + C6 * yz * g[10] + C7 * q * g[13]
             + 2.0f * C9 * xz * g[14] + C5 * s * g[15];
    out[1] = -C1 * g[1] + C2 * (x * g[4] - z * g[5]) - 2.0f * C4 * y * g[8] + C5 * s * g[9] + C6 * xz * g[10] + C7 * q * g[11]
             - 2.0f * C9 * yz * g[14] + 6.0f * C5 * xy * g[15];
    out[2] = C1 * g[2] - C2 * (y * g[5] + x * g[7]) + 2.0f * C3 * z * g[6] + C6 * xy * g[10] - 10.0f * C7 * z * (y * g[11] + x * g[13])
             + C8 * (15.0f * z2 - 3.0f) * g[12] + C9 * (x2 - y2) * g[14];
}

__global__ __launch_bounds__(64) void ngp_points_input_grad_kernel(InputGradArgs a)
{
    __shared__ __attribute__((aligned(16))) char smem[2 * IG_TILE];    // forward: two hidden tiles; chain: the fp32 tile sA over both
    __shared__ float sOut[64];
    __shared__ __attribute__((aligned(16))) float sO[64 * 4];
    static_assert(64 * FB_AS * sizeof(float) <= 2 * IG_TILE, "sA must fit over the two hidden tiles");
    char* sT0 = smem;                       // encoding rows (NGP_XRS) at its head, then the density hidden layer, then the colour net's first
    char* sT1 = smem + IG_TILE;             // colour input rows (NGP_XRS) at its head, then the colour net's second hidden layer
    float* sA = reinterpret_cast<float*>(smem);
    const int lane = threadIdx.x;
    const int fr = lane & 15, kq = lane >> 4;

    for (long pb = (long)blockIdx.x * 64; pb < a.n; pb += (long)gridDim.x * 64) {
        const long p = pb + lane;
        const bool have = p < a.n;
        float gx[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f};
        // ---- the forward, sample for sample; each lane takes its point's three ReLU gates as it goes (the density net's before the colour net
        // overwrites its tile).  False: no gradient arrives at these 64 points: zeros, without the forward
        FieldPoint fp;
        unsigned long long m_hd = 0ull;
        if (field_point_forward(a, p, have, sT0, sT0, sT1, sT0, sT1, sOut, sO, lane, fp, [&] { wave_sync(); m_hd = ngp_relu_mask(sT0, lane); })) {
            const unsigned long long m_h1 = ngp_relu_mask(sT0, lane), m_h2 = ngp_relu_mask(sT1, lane);
            const float (&dO)[3] = fp.dO;
            const float dh0 = fp.dh0;
            bool open[3];                                     // the axis was not clamped: 0 < u_c < 1 before the clamp
#pragma unroll
            for (int c = 0; c < 3; ++c) { const float ur = (fp.x[c] - a.model[c]) / (a.model[3 + c] - a.model[c]); open[c] = ur > 0.f && ur < 1.f; }
            wave_sync();                                      // every lane has its gates: the tiles are dead, sA takes their place
            float* rowA = sA + lane * FB_AS;
            // d2 = relu'(h2) W3[0:3]^T dO (K = 4: column 3 of sA is 0)
#pragma unroll
            for (int c = 0; c < 4; ++c) rowA[c] = c < 3 ? dO[c] : 0.f;
            wave_sync();
            {
                f32x4_t acc[4][4];
                fb_back<1, 4>(acc, sA, a.cw3, 64, 0, lane);
                wave_sync();
                fb_store<4>(sA, acc, FbGateMask{m_h2}, lane);
            }
            wave_sync();
            // d1 = relu'(h1) W2^T d2
            {
                f32x4_t acc[4][4];
                fb_back<16, 4>(acc, sA, a.cw2, 64, 0, lane);
                wave_sync();
                fb_store<4>(sA, acc, FbGateMask{m_h1}, lane);
            }
            wave_sync();
            // colour W1^T d1: columns 0..15 = dsh (kept in sA columns 16..31), columns 16..30 = dout[1..15] (sA columns 1..15); dout[0] = dh0
            {
                f32x4_t acc[4][2];
                fb_back<16, 2>(acc, sA, a.cw1, 32, 0, lane);
                wave_sync();
#pragma unroll
                for (int pt = 0; pt < 4; ++pt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float* row = sA + (pt * 16 + kq * 4 + r) * FB_AS;
                        row[16 + fr] = acc[pt][0][r];
                        if (fr < 15) row[1 + fr] = acc[pt][1][r];
                    }
                rowA[0] = dh0;
            }
            wave_sync();
            // ---- the direction tail, one lane per point
            if (fp.live) ig_sh4_grad(fp.d, rowA + 16, gd);
            // dh = relu'(hd) W2d^T dout (K = 16: columns 16.. of sA are not read)
            {
                f32x4_t acc[4][4];
                fb_back<4, 4>(acc, sA, a.w2, 64, 0, lane);
                wave_sync();
                fb_store<4>(sA, acc, FbGateMask{m_hd}, lane);
            }
            wave_sync();
            // de = W1d^T dh
            {
                f32x4_t acc[4][2];
                fb_back<16, 2>(acc, sA, a.w1, 32, 0, lane);
                wave_sync();
                fb_store<2>(sA, acc, FbGateNone{}, lane);
            }
            wave_sync();
            // ---- the position tail, one lane per point: the encoding's derivative for the row de, as ngp_density_grad_kernel takes it
            if (dh0 != 0.f || dO[0] != 0.f || dO[1] != 0.f || dO[2] != 0.f) {      // (all zero: de is exactly 0, e.g. dL/dsigma alone at a point outside)
                float du[3];
                ngp_encoding_dx(a.table, a.lv, fp.u, rowA, du);
#pragma unroll
                for (int c = 0; c < 3; ++c) gx[c] = open[c] ? du[c] / (a.model[3 + c] - a.model[c]) : 0.f;
            }
            wave_sync();                                      // every lane has read its row of sA: the next pass may write the tiles
        }
        if (have) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (a.grad_x) a.grad_x[p * 3 + c] = gx[c];
                if (a.grad_dir) a.grad_dir[p * 3 + c] = gd[c];
            }
        }
    }
}

struct RayGradArgs {
    long n;
    const int* ray;
    const float *t, *grad_x, *grad_dir;
    long n_rays;
    float *grad_o, *grad_d;
};

__global__ __launch_bounds__(256) void ngp_samples_ray_grad_kernel(RayGradArgs a)
{
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_rays) return;
    long lo = 0, hi = a.n;                                    // the first record whose ray is >= r
    while (lo < hi) {
        const long mid = lo + (hi - lo) / 2;
        if ((long)a.ray[mid] < r) lo = mid + 1; else hi = mid;
    }
    float go[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f};
    for (long k = lo; k < a.n && (long)a.ray[k] == r; ++k) {  // ascending ord: the list's own order
        const float t = a.t[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float g = a.grad_x[k * 3 + c];
            go[c] += g;
            gd[c] += t * g + a.grad_dir[k * 3 + c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { a.grad_o[r * 3 + c] = go[c]; a.grad_d[r * 3 + c] = gd[c]; }
}

extern "C" {

int dreg_ngp_points_input_grad(const float* x, const float* dirs, long n, const void* base16, const void* color16,
                               const uint32_t* offset, const uint32_t* size, const uint32_t* res, const float* scale, const uint32_t* hashed,
                               const float* model_aabb, const float* g_sigma, const float* g_rgb, float* grad_x, float* grad_dir, void* stream)
{
    if (n < 0) return DREG_EINVAL;
    if (n == 0) return DREG_OK;
    InputGradArgs a;
    if (field_fill_points(a, x, dirs, n, base16, color16, offset, size, res, scale, hashed, model_aabb, g_sigma, g_rgb) != DREG_OK) return DREG_EINVAL;
    if (!grad_x && !grad_dir) return DREG_OK;        // nothing to write: nothing is launched
    if (!g_sigma && !g_rgb) {                        // both upstream gradients are zero: the outputs are WRITTEN, as zeros, without a kernel
        if (grad_x && hipMemsetAsync(grad_x, 0, (size_t)n * 3 * sizeof(float), (hipStream_t)stream) != hipSuccess) return DREG_ELAUNCH;
        if (grad_dir && hipMemsetAsync(grad_dir, 0, (size_t)n * 3 * sizeof(float), (hipStream_t)stream) != hipSuccess) return DREG_ELAUNCH;
        return DREG_OK;
    }
    a.grad_x = grad_x; a.grad_dir = grad_dir;
    long waves = (n + 63) / 64;
    if (waves > (1l << 20)) waves = 1l << 20;        // beyond 2^26 points a workgroup takes more than one pass
    hipLaunchKernelGGL(ngp_points_input_grad_kernel, dim3((unsigned)waves), dim3(64), 0, (hipStream_t)stream, a);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

int dreg_ngp_samples_ray_grad(long n, const int* s_ray, const float* s_t, const float* grad_x, const float* grad_dir, long n_rays,
                              float* grad_o, float* grad_d, void* stream)
{
    if (n < 0 || n_rays < 0) return DREG_EINVAL;
    if (n_rays == 0) return DREG_OK;
    if (!grad_o || !grad_d) return DREG_EINVAL;
    if (n > 0 && (!s_ray || !s_t || !grad_x || !grad_dir)) return DREG_EINVAL;
    RayGradArgs a = {n, s_ray, s_t, grad_x, grad_dir, n_rays, grad_o, grad_d};
    hipLaunchKernelGGL(ngp_samples_ray_grad_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

}  // extern "C"
