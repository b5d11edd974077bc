// Joint point-to-plane ICP over a whole registered scene (restatement: tests/scene_icp_restatement.py): all point-to-plane
// residuals of all enabled ordered block pairs (i -> j) minimised over the K - 1 free poses G_b (block b -> the anchor's frame, block 0 fixed)
// at once.  With left perturbations G_b <- exp(xi_b) G_b a residual's Jacobian with respect to xi_j is the negative of the one with respect to
// xi_i, and both are the pair kernel's J' = [q x n, n] of block j's frame moved to the anchor frame by Ad(G_j^-1)^T.  Per iteration, no host
// synchronisation, no atomics:
//   icp_scene_corr_kernel   §3f's correspondence rule (csrc/icp_scan.h) for every enabled ordered pair in ONE launch: the grid is the
//                           concatenation of the pairs' workgroups, a workgroup finds its pair in a table passed by value; per pair the same
//                           30 sums as icp_corr_kernel on (block i's points, block j's index, rel[i][j]), bit for bit;
//   icp_scene_solve_kernel  one workgroup: the pairs' shares in workgroup order, assembly of the 6K x 6K normal equations through the adjoints,
//                           fp64 Cholesky of the 6 (K - 1) free unknowns, pose update, then the next iteration's relative poses rel [K,K,12].
// A first launch of the solve kernel (it = -1) forms rel before iteration 0: 1 + 2 iters launches.  Freezing as §3f.
#include "icp_scan.h"
#include "../../include/dreg_nerf.h"   // dreg_icp_block, DREG_SCENE_MAX_BLOCKS and the signature check of the entry points defined here

constexpr int ICPS_MAXB = DREG_SCENE_MAX_BLOCKS;
constexpr int ICPS_MAXP = ICPS_MAXB * (ICPS_MAXB - 1);
constexpr int ICPS_MAXN = 6 * ICPS_MAXB;

struct IcpSceneBlockDev { const float* src; const float* tp; const float* tn; const int* cell_start; IcpGrid g; int n; };
// wg_end[p]: one past the last workgroup of the p-th enabled pair (INT_MAX beyond the last); pair[p] = i * ICPS_MAXB + j
struct IcpSceneTable { IcpSceneBlockDev blk[ICPS_MAXB]; int wg_end[ICPS_MAXP]; int pair[ICPS_MAXP]; int npairs; int K; };

__global__ __launch_bounds__(ICP_BLOCK) void icp_scene_corr_kernel(IcpSceneTable T, const double* __restrict__ rel, float max_d2, int it,
                                                                   const int* __restrict__ frozen, double* __restrict__ partial)
{
    if (it > 0 && *frozen) return;
    __shared__ double sW[ICP_BLOCK / 64][ICP_NSUM];
    const int bid = (int)blockIdx.x;
    // the workgroup's pair: every table entry is read at a constant index (uniform selects, nothing indexed at run time)
    int w0 = 0, pr = T.pair[0];
#pragma unroll
    for (int k = 0; k + 1 < ICPS_MAXP; ++k)
        if (bid >= T.wg_end[k]) { w0 = T.wg_end[k]; pr = T.pair[k + 1]; }
    const int bi = pr / ICPS_MAXB, bj = pr % ICPS_MAXB;
    const float* src = T.blk[0].src;
    int Ns = T.blk[0].n;
    const float *tp = T.blk[0].tp, *tn = T.blk[0].tn;
    const int* cell_start = T.blk[0].cell_start;
    IcpGrid g = T.blk[0].g;
#pragma unroll
    for (int b = 1; b < ICPS_MAXB; ++b) {
        if (bi == b) { src = T.blk[b].src; Ns = T.blk[b].n; }
        if (bj == b) { tp = T.blk[b].tp; tn = T.blk[b].tn; cell_start = T.blk[b].cell_start; g = T.blk[b].g; }
    }
    const double* pose = rel + (size_t)(bi * T.K + bj) * 12;
    const int i = (bid - w0) * ICP_BLOCK + (int)threadIdx.x;
    double s[ICP_NSUM];
#pragma unroll
    for (int k = 0; k < ICP_NSUM; ++k) s[k] = 0.0;
    if (i < Ns) {
        int best;
        float bd;
        icp_point(src, i, tp, tn, cell_start, g, pose, max_d2, s, best, bd);
    }
    icp_block_reduce(s, sW, partial + (size_t)bid * ICP_NSUM);
}

// rel[i][j] = G_j^-1 G_i: R_ij = R_j^T R_i, t_ij = R_j^T (t_i - t_j), every 3-term sum as (a0 b0 + a1 b1) + a2 b2.  Entry e of [K,K,12].
__device__ __forceinline__ double icp_scene_rel_entry(const double (*G)[12], int K, int e) {
    const int i = e / (12 * K), j = (e / 12) % K, k = e % 12;
    const double *Gi = G[i], *Gj = G[j];
    if (k < 9) {
        const int a = k / 3, b = k % 3;
        return (Gj[a] * Gi[b] + Gj[3 + a] * Gi[3 + b]) + Gj[6 + a] * Gi[6 + b];
    }
    const int a = k - 9;
    return (Gj[a] * (Gi[9] - Gj[9]) + Gj[3 + a] * (Gi[10] - Gj[10])) + Gj[6 + a] * (Gi[11] - Gj[11]);
}

// it = -1: only rel from the poses.  last: the final iteration (rel is then left as this iteration read it).
__global__ __launch_bounds__(64) void icp_scene_solve_kernel(IcpSceneTable T, const double* __restrict__ partial, double* __restrict__ poses, double* __restrict__ rel,
                                                             int* __restrict__ frozen, double* __restrict__ stats, double* __restrict__ pair_sums, int it, int last,
                                                             double tol_rot, double tol_trans, double eps_cond)
{
    const int tid = threadIdx.x, K = T.K;
    __shared__ double G[ICPS_MAXB][12];
    __shared__ int s_status;
    if (it < 0) {
        if (tid < K * 12) G[tid / 12][tid % 12] = poses[tid];
        __syncthreads();
        for (int e = tid; e < K * K * 12; e += 64) rel[e] = icp_scene_rel_entry(G, K, e);
        if (tid == 0) *frozen = 0;
        return;
    }
    double* row = stats + (size_t)it * ICP_STATS;
    if (it > 0 && *frozen) {
        if (tid < ICP_STATS) row[tid] = row[tid - ICP_STATS];
        return;
    }
    __shared__ double S[ICPS_MAXP][ICP_NSUM], H[ICPS_MAXN][ICPS_MAXN], gv[ICPS_MAXN], Lc[ICPS_MAXN][ICPS_MAXN], y[ICPS_MAXN], xi[ICPS_MAXN];
    __shared__ double Ap[6][6], M[6][6], Tm[6][6], bp[6];
    __shared__ int s_wg_end[ICPS_MAXP], s_pair[ICPS_MAXP];
    if (tid < ICPS_MAXP) { s_wg_end[tid] = T.wg_end[tid]; s_pair[tid] = T.pair[tid]; }
    if (tid < K * 12) G[tid / 12][tid % 12] = poses[tid];
    __syncthreads();
    if (tid < ICP_NSUM) {
        for (int p = 0; p < T.npairs; ++p) {
            double a = 0.0;
            for (int k = p ? s_wg_end[p - 1] : 0; k < s_wg_end[p]; ++k) a += partial[(size_t)k * ICP_NSUM + tid];
            S[p][tid] = a;
            if (pair_sums) {
                const int i = s_pair[p] / ICPS_MAXB, j = s_pair[p] % ICPS_MAXB;
                pair_sums[(size_t)(i * K + j) * ICP_NSUM + tid] = a;
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int n = 6 * (K - 1);
        for (int r = 0; r < 6 * K; ++r) {
            gv[r] = 0.0;
            for (int c = 0; c < 6 * K; ++c) H[r][c] = 0.0;
        }
        double count = 0.0, se2 = 0.0, sd2 = 0.0;
        for (int p = 0; p < T.npairs; ++p) {                     // the table lists the enabled pairs in ascending (i, j)
            const int bi = s_pair[p] / ICPS_MAXB, bj = s_pair[p] % ICPS_MAXB;
            const double* Sp = S[p];
            count += Sp[29]; se2 += Sp[27]; sd2 += Sp[28];
            int k = 0;
            for (int r = 0; r < 6; ++r)
                for (int c = r; c < 6; ++c) { Ap[r][c] = Sp[k]; Ap[c][r] = Sp[k]; ++k; }
            for (int r = 0; r < 6; ++r) bp[r] = Sp[21 + r];
            // M = Ad(G_j^-1) = [[R_j^T, 0], [-R_j^T [t_j]x, R_j^T]] on (omega, v); row r of R^T [t]x is (column r of R) x t
            const double* Gj = G[bj];
            for (int r = 0; r < 3; ++r) {
                const double c0 = Gj[r], c1 = Gj[3 + r], c2 = Gj[6 + r];           // column r of R_j = row r of R_j^T
                const double x0 = c1 * Gj[11] - c2 * Gj[10], x1 = c2 * Gj[9] - c0 * Gj[11], x2 = c0 * Gj[10] - c1 * Gj[9];   // R_col_r x t
                M[r][0] = c0; M[r][1] = c1; M[r][2] = c2; M[r][3] = 0.0; M[r][4] = 0.0; M[r][5] = 0.0;
                M[3 + r][0] = -x0; M[3 + r][1] = -x1; M[3 + r][2] = -x2; M[3 + r][3] = c0; M[3 + r][4] = c1; M[3 + r][5] = c2;
            }
            for (int r = 0; r < 6; ++r)                           // Tm = A' M
                for (int c = 0; c < 6; ++c) {
                    double a = 0.0;
                    for (int m = 0; m < 6; ++m) a += Ap[r][m] * M[m][c];
                    Tm[r][c] = a;
                }
            for (int r = 0; r < 6; ++r) {                         // A = M^T Tm, b = M^T b'
                double bb = 0.0;
                for (int m = 0; m < 6; ++m) bb += M[m][r] * bp[m];
                gv[6 * bi + r] += bb;
                gv[6 * bj + r] -= bb;
                for (int c = 0; c < 6; ++c) {
                    double a = 0.0;
                    for (int m = 0; m < 6; ++m) a += M[m][r] * Tm[m][c];
                    H[6 * bi + r][6 * bi + c] += a;
                    H[6 * bj + r][6 * bj + c] += a;
                    H[6 * bi + r][6 * bj + c] -= a;
                    H[6 * bj + r][6 * bi + c] -= a;
                }
            }
        }
        // block 0's rows and columns are dropped: unknown u of the reduced system is row 6 + u of H
        int status = 0;
        double ratio = 0.0, nw = 0.0, nv = 0.0;
        if (count < (double)n) status = 2;
        else {
            ratio = 1.0 / 0.0;
            for (int c = 0; c < n && status == 0; ++c) {
                const double acc = H[6 + c][6 + c];
                double d = acc;
                for (int j = 0; j < c; ++j) d -= Lc[c][j] * Lc[c][j];
                const double rt = acc > 0.0 ? d / acc : 0.0;
                ratio = rt < ratio ? rt : ratio;
                if (!(acc > 0.0) || !(d > eps_cond * acc)) { status = 3; break; }
                const double l = sqrt(d);
                Lc[c][c] = l;
                for (int i = c + 1; i < n; ++i) {
                    double v = H[6 + i][6 + c];
                    for (int j = 0; j < c; ++j) v -= Lc[i][j] * Lc[c][j];
                    Lc[i][c] = v / l;
                }
            }
        }
        if (status == 0) {
            for (int i = 0; i < n; ++i) {                 // L y = -g
                double v = -gv[6 + i];
                for (int j = 0; j < i; ++j) v -= Lc[i][j] * y[j];
                y[i] = v / Lc[i][i];
            }
            for (int i = n - 1; i >= 0; --i) {            // L^T xi = y
                double v = y[i];
                for (int j = i + 1; j < n; ++j) v -= Lc[j][i] * xi[j];
                xi[i] = v / Lc[i][i];
            }
            for (int b = 1; b < K; ++b) {
                const double* x = xi + 6 * (b - 1);
                const double w0 = x[0], w1 = x[1], w2 = x[2];
                const double bw = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
                const double bv = sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]);
                nw = bw > nw ? bw : nw;
                nv = bv > nv ? bv : nv;
                double E[3][3];
                icp_exp_so3(w0, w1, w2, bw, E);
                icp_apply_update(E, x[3], x[4], x[5], G[b]);
                for (int k = 0; k < 12; ++k) poses[12 * b + k] = G[b][k];
            }
            if (nw < tol_rot && nv < tol_trans) status = 1;
        }
        row[0] = count; row[1] = se2; row[2] = sd2; row[3] = nw; row[4] = nv; row[5] = ratio; row[6] = (double)status;
        *frozen = status != 0 ? 1 : 0;
        s_status = status;
    }
    __syncthreads();
    if (s_status == 0 && !last)
        for (int e = tid; e < K * K * 12; e += 64) rel[e] = icp_scene_rel_entry(G, K, e);
}

extern "C" {

static bool icp_scene_pair_on(const uint8_t* pair_mask, int K, int i, int j) { return i != j && (!pair_mask || pair_mask[i * K + j]); }

// workspace: one share of the 30 sums per workgroup of icp_scene_corr_kernel, rel [K,K,12], then the freeze flag
size_t dreg_icp_scene_workspace_bytes(int n_blocks, const dreg_icp_block* blocks, const uint8_t* pair_mask)
{
    if (n_blocks < 2 || n_blocks > ICPS_MAXB || !blocks) return 0;
    size_t nwg = 0;
    for (int i = 0; i < n_blocks; ++i) {
        if (blocks[i].n < 1) return 0;
        for (int j = 0; j < n_blocks; ++j)
            if (icp_scene_pair_on(pair_mask, n_blocks, i, j)) nwg += ((size_t)blocks[i].n + ICP_BLOCK - 1) / ICP_BLOCK;
    }
    return (nwg * ICP_NSUM + (size_t)n_blocks * n_blocks * 12 + 1) * sizeof(double);
}

int dreg_icp_scene_refine(int n_blocks, const dreg_icp_block* blocks, const uint8_t* pair_mask, double* poses, float max_dist, int iters,
                          double tol_rot, double tol_trans, double eps_cond, double* stats, double* pair_sums, double* rel_out,
                          void* workspace, size_t workspace_bytes, void* stream)
{
    if (n_blocks < 2 || n_blocks > ICPS_MAXB || !blocks || !poses || !workspace || iters < 0) return DREG_EINVAL;
    if (iters > 0 && !stats) return DREG_EINVAL;
    if (!(max_dist >= 0.f)) return DREG_EINVAL;
    const int K = n_blocks;
    IcpSceneTable T;
    for (int b = 0; b < ICPS_MAXB; ++b) {
        const dreg_icp_block& B = blocks[b < K ? b : 0];
        if (b < K) {
            if (B.n < 1 || !B.src || !B.tgt_points || !B.tgt_normals || !B.cell_start) return DREG_EINVAL;
            if (!(B.cell > 0.f) || B.cell < max_dist || B.nx <= 0 || B.ny <= 0 || B.nz <= 0 || (long long)B.nx * B.ny * B.nz > (1ll << 24)) return DREG_EINVAL;
        }
        IcpSceneBlockDev& D = T.blk[b];
        D.src = B.src; D.tp = B.tgt_points; D.tn = B.tgt_normals; D.cell_start = B.cell_start; D.n = B.n;
        for (int c = 0; c < 3; ++c) D.g.lo[c] = B.grid_lo[c];
        D.g.cell = B.cell; D.g.dim[0] = B.nx; D.g.dim[1] = B.ny; D.g.dim[2] = B.nz;
    }
    const size_t need = dreg_icp_scene_workspace_bytes(K, blocks, pair_mask);
    if (need == 0 || workspace_bytes < need || ((uintptr_t)workspace & 7)) return DREG_EINVAL;
    long long nwg = 0;
    int np = 0;
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j)
            if (icp_scene_pair_on(pair_mask, K, i, j)) {
                nwg += (blocks[i].n + ICP_BLOCK - 1) / ICP_BLOCK;
                T.wg_end[np] = (int)nwg;
                T.pair[np] = i * ICPS_MAXB + j;
                ++np;
            }
    if (nwg > 0x7fffffffll) return DREG_EINVAL;
    for (int p = np; p < ICPS_MAXP; ++p) { T.wg_end[p] = 0x7fffffff; T.pair[p] = 1; }
    T.npairs = np;
    T.K = K;
    double* partial = (double*)workspace;
    double* rel_ws = partial + (size_t)nwg * ICP_NSUM;
    int* frozen = (int*)(rel_ws + (size_t)K * K * 12);
    double* rel = rel_out ? rel_out : rel_ws;
    const float max_d2 = max_dist * max_dist;
    hipLaunchKernelGGL(icp_scene_solve_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, T, (const double*)partial, poses, rel, frozen, stats, pair_sums, -1, 0,
                       tol_rot, tol_trans, eps_cond);
    for (int it = 0; it < iters; ++it) {
        if (nwg > 0)
            hipLaunchKernelGGL(icp_scene_corr_kernel, dim3((unsigned)nwg), dim3(ICP_BLOCK), 0, (hipStream_t)stream, T, (const double*)rel, max_d2, it,
                               (const int*)frozen, partial);
        hipLaunchKernelGGL(icp_scene_solve_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, T, (const double*)partial, poses, rel, frozen, stats, pair_sums, it,
                           it == iters - 1 ? 1 : 0, tol_rot, tol_trans, eps_cond);
    }
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

}  // extern "C"
