// Point-to-plane ICP refinement of a predicted pose (the reference's refine_registration, conerf/geometry/global_registration.py:85-93, which
// runs open3d's registration_icp with TransformationEstimationPointToPlane on the host; its call is commented out as too slow).  Rule and tests:
// DESIGN.md §3f, tests/icp_restatement.py.  Two kernels per iteration, no host synchronisation between iterations, no atomics:
//   icp_corr_kernel   one lane per source point: q = R p + t (fp32), exact nearest neighbour among the 27 cells of a uniform grid over the
//                     target (dreg_nerf_amd/icp.py TargetIndex), the point-to-plane residual e = n.(q - p_t) with J = [q x n, n], and the
//                     workgroup's share of the 30 sums of the normal equations in fp64 (fixed reduction order);
//   icp_solve_kernel  one workgroup: adds the shares in workgroup order, fp64 Cholesky of the 6x6, xi = -A^-1 b, pose <- exp(xi) pose.
// The pose (fp64 [12]: R row-major, then t) stays on the device.  A run freezes on convergence (status 1), on fewer than 6 correspondences
// (2) or on a degenerate system (3); from then on both kernels return at once and the stats rows repeat the last one.
#include "icp_scan.h"

// one source point's work (transform, cell, 27-cell scan, gate, e, J, the 30 terms) and the reduction: csrc/icp_scan.h
__global__ __launch_bounds__(ICP_BLOCK) void icp_corr_kernel(const float* __restrict__ src, int Ns, const float* __restrict__ tp, const float* __restrict__ tn,
                                                             const int* __restrict__ perm, const int* __restrict__ cell_start, IcpGrid g,
                                                             const double* __restrict__ pose, float max_d2, int it, const int* __restrict__ frozen,
                                                             double* __restrict__ partial, int* __restrict__ corr, float* __restrict__ dist2)
{
    if (it > 0 && *frozen) return;
    __shared__ double sW[ICP_BLOCK / 64][ICP_NSUM];
    const int i = (int)blockIdx.x * ICP_BLOCK + (int)threadIdx.x;
    double s[ICP_NSUM];
#pragma unroll
    for (int k = 0; k < ICP_NSUM; ++k) s[k] = 0.0;
    if (i < Ns) {
        int best;
        float bd;
        const bool ok = icp_point(src, i, tp, tn, cell_start, g, pose, max_d2, s, best, bd);
        if (corr) corr[i] = ok ? perm[best] : -1;
        if (dist2) dist2[i] = ok ? bd : __builtin_inff();
    }
    icp_block_reduce(s, sW, partial + (size_t)blockIdx.x * ICP_NSUM);
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
        double E[3][3];
        icp_exp_so3(w0, w1, w2, nw, E);
        icp_apply_update(E, xi[3], xi[4], xi[5], pose);
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
