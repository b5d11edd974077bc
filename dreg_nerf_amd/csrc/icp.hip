// Point-to-plane ICP refinement of a predicted pose (the reference's refine_registration, conerf/geometry/global_registration.py:85-93, which
// runs open3d's registration_icp with TransformationEstimationPointToPlane on the host; its call is commented out as too slow).  Rule and tests:
// DESIGN.md §3f, tests/icp_restatement.py.  Two kernels per iteration, no host synchronisation between iterations, no atomics:
//   icp_corr_kernel   one lane per source point: q = R p + t (fp32), exact nearest neighbour among the 27 cells of a uniform grid over the
//                     target (dreg_nerf_amd/icp.py TargetIndex), the point-to-plane residual e = n.(q - p_t) with J = [q x n, n], and the
//                     workgroup's share of the 30 sums of the normal equations in fp64 (fixed reduction order);
//   icp_solve_kernel  one workgroup: adds the shares in workgroup order, fp64 Cholesky of the 6x6, xi = -A^-1 b, pose <- exp(xi) pose.
// The pose (fp64 [12]: R row-major, then t) stays on the device.  A run freezes on convergence (status 1), on fewer than 6 correspondences
// (2) or on a degenerate system (3); from then on both kernels return at once and the stats rows repeat the last one.
#include "common.h"

constexpr int ICP_NSUM = 30;      // 21 of J^T J (upper triangle, row-major), 6 of J^T e, sum e^2, sum d^2, count
constexpr int ICP_BLOCK = 256;
constexpr int ICP_STATS = 7;      // count, sum e^2, sum d^2, |omega|, |v|, smallest pivot ratio, status

struct IcpGrid { float lo[3]; float cell; int dim[3]; };

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(ICP_BLOCK) void icp_corr_kernel(const float* __restrict__ src, int Ns, const float* __restrict__ tp, const float* __restrict__ tn,
                                                             const int* __restrict__ perm, const int* __restrict__ cell_start, IcpGrid g,
                                                             const double* __restrict__ pose, float max_d2, int it, const int* __restrict__ frozen,
                                                             double* __restrict__ partial, int* __restrict__ corr, float* __restrict__ dist2)
{
    if (it > 0 && *frozen) return;
    __shared__ double sW[ICP_BLOCK / 64][ICP_NSUM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = (int)blockIdx.x * ICP_BLOCK + tid;
    double s[ICP_NSUM];
#pragma unroll
    for (int k = 0; k < ICP_NSUM; ++k) s[k] = 0.0;
    if (i < Ns) {
        float P[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) P[k] = (float)pose[k];
        const float p0 = src[(size_t)i * 3], p1 = src[(size_t)i * 3 + 1], p2 = src[(size_t)i * 3 + 2];
        float q[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = ((P[3 * c] * p0 + P[3 * c + 1] * p1) + P[3 * c + 2] * p2) + P[9 + c];
        // q's cell; outside the grid (a NaN included) there is no target point within a cell's width: no correspondence
        bool in = true;
        int ci[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float fc = floorf((q[c] - g.lo[c]) / g.cell);
            in = in && (fc >= 0.f) && (fc < (float)g.dim[c]);
            ci[c] = in ? (int)fc : 0;
        }
        int best = -1;
        float bd = __builtin_inff();
        if (in) {
            const int x0 = max(ci[0] - 1, 0), x1 = min(ci[0] + 1, g.dim[0] - 1);
            for (int dz = -1; dz <= 1; ++dz) {
                const int z = ci[2] + dz;
                if (z < 0 || z >= g.dim[2]) continue;
                for (int dy = -1; dy <= 1; ++dy) {
                    const int y = ci[1] + dy;
                    if (y < 0 || y >= g.dim[1]) continue;
                    // the cells x0..x1 of this row are consecutive ids: one range of the sorted points, in ascending cell id
                    const int c0 = x0 + g.dim[0] * (y + g.dim[1] * z);
                    const int j1 = cell_start[c0 + (x1 - x0) + 1];
                    for (int j = cell_start[c0]; j < j1; ++j) {
                        const float r0 = q[0] - tp[(size_t)j * 3], r1 = q[1] - tp[(size_t)j * 3 + 1], r2 = q[2] - tp[(size_t)j * 3 + 2];
                        const float d2 = (r0 * r0 + r1 * r1) + r2 * r2;
                        if (d2 < bd) { bd = d2; best = j; }
                    }
                }
            }
        }
        bool ok = best >= 0 && bd <= max_d2;
        float n[3] = {0.f, 0.f, 0.f}, r[3] = {0.f, 0.f, 0.f};
        if (ok) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { n[c] = tn[(size_t)best * 3 + c]; r[c] = q[c] - tp[(size_t)best * 3 + c]; }
            ok = !(n[0] == 0.f && n[1] == 0.f && n[2] == 0.f);
        }
        if (corr) corr[i] = ok ? perm[best] : -1;
        if (dist2) dist2[i] = ok ? bd : __builtin_inff();
        if (ok) {
            const float e = (n[0] * r[0] + n[1] * r[1]) + n[2] * r[2];
            const float Jf[6] = {q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0], n[0], n[1], n[2]};
            double J[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) J[a] = (double)Jf[a];
            const double ed = (double)e;
            int k = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = a; b < 6; ++b) s[k++] = J[a] * J[b];
#pragma unroll
            for (int a = 0; a < 6; ++a) s[21 + a] = J[a] * ed;
            s[27] = ed * ed; s[28] = (double)bd; s[29] = 1.0;
        }
    }
    // fixed order: butterfly within the wave (every lane ends with the same sum), then the waves in order
#pragma unroll
    for (int k = 0; k < ICP_NSUM; ++k) s[k] = wave_sum_f64(s[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < ICP_NSUM; ++k) sW[wave][k] = s[k];
    }
    __syncthreads();
    if (tid < ICP_NSUM) {
        double a = sW[0][tid];
#pragma unroll
        for (int w = 1; w < ICP_BLOCK / 64; ++w) a += sW[w][tid];
        partial[(size_t)blockIdx.x * ICP_NSUM + tid] = a;
    }
}

__global__ __launch_bounds__(64) void icp_solve_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ pose, int* __restrict__ frozen,
                                                       double* __restrict__ stats, double* __restrict__ sums, int it, double tol_rot, double tol_trans,
                                                       double eps_cond)
{
    const int tid = threadIdx.x;
    double* row = stats + (size_t)it * ICP_STATS;
    if (it > 0 && *frozen) {
        if (tid < ICP_STATS) row[tid] = row[tid - ICP_STATS];
        return;
    }
    __shared__ double S[ICP_NSUM], A[6][6], Lc[6][6], b[6], y[6], xi[6];
    if (tid < ICP_NSUM) {
        double a = 0.0;
        for (int k = 0; k < nblk; ++k) a += partial[(size_t)k * ICP_NSUM + tid];
        S[tid] = a;
        if (sums) sums[tid] = a;
    }
    __syncthreads();
    if (tid != 0) return;
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) { A[i][j] = S[k]; A[j][i] = S[k]; ++k; }
    for (int i = 0; i < 6; ++i) b[i] = S[21 + i];
    const double count = S[29];
    int status = 0;
    double ratio = 0.0, nw = 0.0, nv = 0.0;
    if (count < 6.0) status = 2;
    else {
        ratio = 1.0 / 0.0;
        for (int c = 0; c < 6 && status == 0; ++c) {
            double d = A[c][c];
            for (int j = 0; j < c; ++j) d -= Lc[c][j] * Lc[c][j];
            const double rt = A[c][c] > 0.0 ? d / A[c][c] : 0.0;
            ratio = rt < ratio ? rt : ratio;
            if (!(A[c][c] > 0.0) || !(d > eps_cond * A[c][c])) { status = 3; break; }
            const double l = sqrt(d);
            Lc[c][c] = l;
            for (int i = c + 1; i < 6; ++i) {
                double v = A[i][c];
                for (int j = 0; j < c; ++j) v -= Lc[i][j] * Lc[c][j];
                Lc[i][c] = v / l;
            }
        }
    }
    if (status == 0) {
        for (int i = 0; i < 6; ++i) {                 // L y = -b
            double v = -b[i];
            for (int j = 0; j < i; ++j) v -= Lc[i][j] * y[j];
            y[i] = v / Lc[i][i];
        }
        for (int i = 5; i >= 0; --i) {                // L^T xi = y
            double v = y[i];
            for (int j = i + 1; j < 6; ++j) v -= Lc[j][i] * xi[j];
            xi[i] = v / Lc[i][i];
        }
        const double w0 = xi[0], w1 = xi[1], w2 = xi[2];
        nw = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
        nv = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
        // Rodrigues: E = I + a K + c K^2, a = sin(th)/th, c = (1 - cos th)/th^2 = (sin(th/2)/(th/2))^2 / 2 (no cancellation at small th)
        double a = 1.0, c = 0.5;
        if (nw > 0.0) { a = sin(nw) / nw; const double h = sin(0.5 * nw) / (0.5 * nw); c = 0.5 * h * h; }
        const double K[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
        double E[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const double k2 = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
                E[i][j] = ((i == j ? 1.0 : 0.0) + a * K[i][j]) + c * k2;
            }
        double Pn[12];
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) Pn[3 * i + j] = (E[i][0] * pose[j] + E[i][1] * pose[3 + j]) + E[i][2] * pose[6 + j];
            Pn[9 + i] = ((E[i][0] * pose[9] + E[i][1] * pose[10]) + E[i][2] * pose[11]) + xi[3 + i];
        }
        for (int i = 0; i < 12; ++i) pose[i] = Pn[i];
        if (nw < tol_rot && nv < tol_trans) status = 1;
    }
    row[0] = count; row[1] = S[27]; row[2] = S[28]; row[3] = nw; row[4] = nv; row[5] = ratio; row[6] = (double)status;
    *frozen = status != 0 ? 1 : 0;
}

extern "C" {

// workspace: one share of the 30 sums per workgroup of icp_corr_kernel, then the freeze flag
size_t dreg_icp_workspace_bytes(int Ns, int iters)
{
    if (Ns < 0 || iters < 0) return 0;
    const size_t nblk = ((size_t)Ns + ICP_BLOCK - 1) / ICP_BLOCK;
    return (nblk * ICP_NSUM + 1) * sizeof(double);
}

int dreg_icp_refine(const float* src, int Ns, const float* tgt_points, const float* tgt_normals, const int* perm, const int* cell_start, int Nt,
                    const float* grid_lo, float cell, int nx, int ny, int nz, double* pose, float max_dist, int iters,
                    double tol_rot, double tol_trans, double eps_cond, double* stats, double* sums, int* corr, float* dist2,
                    void* workspace, size_t workspace_bytes, void* stream)
{
    if (Ns < 0 || Nt <= 0 || iters < 0 || (Ns > 0 && !src) || !tgt_points || !tgt_normals || !perm || !cell_start || !grid_lo || !pose || !workspace)
        return DREG_EINVAL;
    if (iters > 0 && !stats) return DREG_EINVAL;
    if (!(cell > 0.f) || !(max_dist >= 0.f) || cell < max_dist || nx <= 0 || ny <= 0 || nz <= 0 || (long long)nx * ny * nz > (1ll << 24)) return DREG_EINVAL;
    if (workspace_bytes < dreg_icp_workspace_bytes(Ns, iters) || ((uintptr_t)workspace & 7)) return DREG_EINVAL;
    const int nblk = (Ns + ICP_BLOCK - 1) / ICP_BLOCK;
    double* partial = (double*)workspace;
    int* frozen = (int*)(partial + (size_t)nblk * ICP_NSUM);
    IcpGrid g;
    for (int c = 0; c < 3; ++c) g.lo[c] = grid_lo[c];
    g.cell = cell; g.dim[0] = nx; g.dim[1] = ny; g.dim[2] = nz;
    const float max_d2 = max_dist * max_dist;
    for (int it = 0; it < iters; ++it) {
        if (nblk > 0)
            hipLaunchKernelGGL(icp_corr_kernel, dim3(nblk), dim3(ICP_BLOCK), 0, (hipStream_t)stream, src, Ns, tgt_points, tgt_normals, perm, cell_start, g,
                               (const double*)pose, max_d2, it, (const int*)frozen, partial, corr, dist2);
        hipLaunchKernelGGL(icp_solve_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partial, nblk, pose, frozen, stats, sums, it,
                           tol_rot, tol_trans, eps_cond);
    }
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

}  // extern "C"
