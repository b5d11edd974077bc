// Density of a NeRF block's field together with its gradient in world space (restatement: tests/ngp_grad_restatement.py): the
// surface normals of the block's point cloud, analytically, for the ICP target (dreg_nerf_amd/icp.py) and for point_cloud.ply.
// The forward is the field's own (ngp_field.h: ngp_unit_cube, ngp_level_features, ngp_density_mlp, called as they are), so the density equals
// dreg_ngp_density_fwd_ws's bit for bit.  The gradient is the straight-through one (the fp16 roundings taken as identity):
//   g_j = w2[0][j] where the stored fp16 hidden activation h_j > 0, else 0;   f_i = sum_j w1[j][i] g_j  (fp32, j ascending);
//   du_c = sum_l scale_l sum_corners (s_c w_a w_b) (f_2l t_0 + f_2l+1 t_1),   s_c = +-1 by the corner's side on axis c, w_a, w_b the trilinear
//   weights of the other two axes, t the corner's two table entries;   grad_c = sigma du_c / (hi_c - lo_c), zero outside the aabb.
// One point per lane, one wave per 64 points and per workgroup, as ngp_density_kernel.  f = W1^T g comes from LDS-staged weights (every lane reads
// the same row: a broadcast), 32 accumulators per lane; it then goes to the lane's own row of the hidden tile, from where the level loop reads two
// values per level.  The ReLU mask and the encoding's derivative (the corner loop of every level, run a second time with a hook that accumulates
// the three derivatives) are ngp_field.h's ngp_relu_mask and ngp_encoding_dx, which the input gradients of field_input_grad.hip call as well.
#include "ngp_field.h"

__global__ __launch_bounds__(64) void ngp_density_grad_kernel(const float* __restrict__ x, const _Float16* __restrict__ table,
                                                              const _Float16* __restrict__ w1, const _Float16* __restrict__ w2,
                                                              float* __restrict__ density, float* __restrict__ grad, unsigned long long* __restrict__ relu_mask,
                                                              NgpLevels lv, float lo0, float lo1, float lo2, float hi0, float hi1, float hi2, int Np)
{
    constexpr int XRS = NGP_XRS, HRS = NGP_HRS;
    // the hidden tile (the encoded input aliases its head until the first layer has read it), the density of every point of the wave, w1 and w2[0]
    __shared__ __attribute__((aligned(16))) char smem[64 * HRS];
    __shared__ float sD[64];
    __shared__ __attribute__((aligned(16))) _Float16 sW1[64 * 32];
    __shared__ _Float16 sW2[64];
    const int lane = threadIdx.x & 63;
    char* sH = smem;
    char* sX = sH;
    const int p0 = (int)blockIdx.x * 64;
    const int p = p0 + lane;
    const float lo[3] = {lo0, lo1, lo2}, hi[3] = {hi0, hi1, hi2};
    float u[3] = {0.f, 0.f, 0.f};
    bool inside = false;
    if (p < Np) {
        const float xp[3] = {x[(size_t)p * 3], x[(size_t)p * 3 + 1], x[(size_t)p * 3 + 2]};
        inside = ngp_unit_cube(xp, lo, hi, 0, u);
    }
    // stage the first layer's weights (fp16 [64][32]: 64 bytes per lane) and the density row of the second
#pragma unroll
    for (int k = 0; k < 4; ++k) reinterpret_cast<uint4*>(sW1)[lane * 4 + k] = reinterpret_cast<const uint4*>(w1)[lane * 4 + k];
    sW2[lane] = w2[lane];
    for (int l = 0; l < 16; ++l) {
        float f0, f1;
        ngp_level_features(table, lv, l, u, f0, f1);
        _Float16* xr = reinterpret_cast<_Float16*>(sX + lane * XRS);
        xr[2 * l] = (_Float16)f0; xr[2 * l + 1] = (_Float16)f1;
    }
    NgpDensityW dw;
    ngp_load_density_w(dw, w1, w2, lane);
    const int fr = lane & 15, kg = lane >> 4;
    ngp_density_mlp(dw, sX, sH, lane, [&](int rb, const f32x4_t& o) {
        if (fr == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) sD[rb * 16 + kg * 4 + r] = (float)(_Float16)o[r];      // the density logit as ngp_density_kernel rounds it
        }
    });
    wave_sync();
    const float sigma = __expf(sD[lane] - 1.f) * (inside ? 1.f : 0.f);
    const unsigned long long mask = ngp_relu_mask(sH, lane);      // bit j = the stored fp16 h_j > 0
    // f = W1^T g: products of two fp16 values are exact in fp32, the 64 additions round
    float f[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) f[i] = 0.f;
#pragma unroll 2
    for (int j = 0; j < 64; ++j) {
        const float g = ((mask >> j) & 1ull) ? (float)sW2[j] : 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const f16x8_t wv = *reinterpret_cast<const f16x8_t*>(sW1 + j * 32 + k * 8);
#pragma unroll
            for (int i = 0; i < 8; ++i) f[k * 8 + i] += (float)wv[i] * g;
        }
    }
    // park f in the lane's own row (its 64 fp16 activations are consumed): 32 fp32 = the row's 128 bytes
    float* fr_row = reinterpret_cast<float*>(sH + lane * HRS);
#pragma unroll
    for (int i = 0; i < 32; ++i) fr_row[i] = f[i];
    float du[3];
    ngp_encoding_dx(table, lv, u, fr_row, du);
    if (p < Np) {
        density[p] = sigma;
#pragma unroll
        for (int c = 0; c < 3; ++c) grad[(size_t)p * 3 + c] = inside ? (sigma * du[c]) / (hi[c] - lo[c]) : 0.f;
        if (relu_mask) relu_mask[p] = mask;
    }
}

extern "C" {

// x fp32 [Np,3] world; table / w1 / w2 / the five level arrays / aabb as for dreg_ngp_density_fwd.  density fp32 [Np] (= dreg_ngp_density_fwd_ws's, bit
// for bit), grad fp32 [Np,3] = d density / d x (zero outside the aabb), relu_mask (optional) uint64 [Np]: bit j = hidden unit j of the density net active.
int dreg_ngp_density_grad(const float* x, const void* table, const void* w1, const void* w2, float* density, float* grad, unsigned long long* relu_mask,
                          const uint32_t* offset, const uint32_t* size, const uint32_t* res, const float* scale, const uint32_t* hashed,
                          const float* aabb, int Np, int contract, void* stream)
{
    if (contract != 0 || Np < 0 || !table || !w1 || !w2 || !offset || !size || !res || !scale || !hashed || !aabb) return DREG_EINVAL;
    if (Np > 0 && (!x || !density || !grad)) return DREG_EINVAL;
    if (Np == 0) return DREG_OK;
    NgpLevels lv;
    ngp_fill_levels(lv, offset, size, res, scale, hashed);
    hipLaunchKernelGGL(ngp_density_grad_kernel, dim3((Np + 63) / 64), dim3(64), 0, (hipStream_t)stream, x, (const _Float16*)table, (const _Float16*)w1,
                       (const _Float16*)w2, density, grad, relu_mask, lv, aabb[0], aabb[1], aabb[2], aabb[3], aabb[4], aabb[5], Np);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

}  // extern "C"
