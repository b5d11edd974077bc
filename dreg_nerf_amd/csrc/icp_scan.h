// One source point's work in the point-to-plane ICP kernels, and the reduction of the 30 sums: DESIGN.md §3f's rule stated once, for
// icp_corr_kernel (csrc/icp.hip, one pair) and icp_scene_corr_kernel (csrc/icp_scene.hip, every ordered pair of a scene in one launch).  Both
// form, per pair, the same 30 sums bit for bit (tests/test_hip_icp.py, tests/test_hip_scene_icp.py).
#pragma once
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

// q = R p + t with the fp64 pose rounded to fp32
__device__ __forceinline__ void icp_transform(const float* __restrict__ src, int i, const double* __restrict__ pose, float (&q)[3]) {
    float P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = (float)pose[k];
    const float p0 = src[(size_t)i * 3], p1 = src[(size_t)i * 3 + 1], p2 = src[(size_t)i * 3 + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = ((P[3 * c] * p0 + P[3 * c + 1] * p1) + P[3 * c + 2] * p2) + P[9 + c];
}

// exact nearest neighbour of q among the 27 cells around q's cell: the sorted index of the target point (-1: none) and its squared distance
__device__ __forceinline__ int icp_scan(const float (&q)[3], const float* __restrict__ tp, const int* __restrict__ cell_start, const IcpGrid& g, float& bd) {
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
    bd = __builtin_inff();
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
    return best;
}

// The whole of one source point: s (zeroed by the caller) receives its 30 terms when it has a correspondence.  Returns whether it has one;
// best / bd: the sorted index of the nearest target point (-1: none) and its squared distance.
__device__ __forceinline__ bool icp_point(const float* __restrict__ src, int i, const float* __restrict__ tp, const float* __restrict__ tn,
                                          const int* __restrict__ cell_start, const IcpGrid& g, const double* __restrict__ pose, float max_d2,
                                          double (&s)[ICP_NSUM], int& best, float& bd) {
    float q[3];
    icp_transform(src, i, pose, q);
    best = icp_scan(q, tp, cell_start, g, bd);
    bool ok = best >= 0 && bd <= max_d2;
    float n[3] = {0.f, 0.f, 0.f}, r[3] = {0.f, 0.f, 0.f};
    if (ok) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { n[c] = tn[(size_t)best * 3 + c]; r[c] = q[c] - tp[(size_t)best * 3 + c]; }
        ok = !(n[0] == 0.f && n[1] == 0.f && n[2] == 0.f);
    }
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
    return ok;
}

// The workgroup's share of the 30 sums, written to out[30].  Fixed order: butterfly within the wave (every lane ends with the same sum), then
// the waves in order.  sW: ICP_BLOCK / 64 rows of shared memory; every thread of the workgroup calls this.
__device__ __forceinline__ void icp_block_reduce(double (&s)[ICP_NSUM], double (*sW)[ICP_NSUM], double* __restrict__ out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
        out[tid] = a;
    }
}

// exp(w) for a rotation vector w, row-major.  Rodrigues: E = I + a K + c K^2, a = sin(th)/th, c = (1 - cos th)/th^2 = (sin(th/2)/(th/2))^2 / 2
// (no cancellation at small th); nw = |w| as the caller formed it.
__device__ __forceinline__ void icp_exp_so3(double w0, double w1, double w2, double nw, double (&E)[3][3]) {
    double a = 1.0, c = 0.5;
    if (nw > 0.0) { a = sin(nw) / nw; const double h = sin(0.5 * nw) / (0.5 * nw); c = 0.5 * h * h; }
    const double K[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double k2 = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
            E[i][j] = ((i == j ? 1.0 : 0.0) + a * K[i][j]) + c * k2;
        }
}

// pose <- exp(omega) pose for a pose of 12 fp64 (R row-major, then t): R <- E R, t <- E t + v
__device__ __forceinline__ void icp_apply_update(const double (&E)[3][3], double v0, double v1, double v2, double* __restrict__ pose) {
    const double v[3] = {v0, v1, v2};
    double Pn[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Pn[3 * i + j] = (E[i][0] * pose[j] + E[i][1] * pose[3 + j]) + E[i][2] * pose[6 + j];
        Pn[9 + i] = ((E[i][0] * pose[9] + E[i][1] * pose[10]) + E[i][2] * pose[11]) + v[i];
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) pose[i] = Pn[i];
}
