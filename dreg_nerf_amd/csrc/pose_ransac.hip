// Robust pose from correspondences: hypothesise-and-verify over minimal samples (RANSAC) next to the least-squares weighted Kabsch solve.
// Rule and tests: DESIGN.md §3g, tests/pose_ransac_restatement.py.  Three kernels, no atomics, no floating-point sums, no host synchronisation:
//   ransac_score_kernel   one hypothesis per lane: the lane builds (R, t) from its triplet (triad, 12 registers) and counts the correspondences
//                         of its workgroup's slice with |R a + t - b|^2 <= thresh^2.  The slice is staged through LDS in tiles of 64 rows of 8
//                         floats; every lane reads the same row (two 16-byte reads of one address: a broadcast, no bank conflict).  The count
//                         of (hypothesis, slice) goes to its own int32 cell of the workspace (-1 for an invalid hypothesis);
//   ransac_select_kernel  one workgroup: adds the cells of each hypothesis in slice order, largest count with the smallest index on a tie,
//                         writes best / pose / status (and the optional per-hypothesis counts and poses);
//   pose_inliers_kernel   one workgroup: mask and count of a pose that is on the device, same d^2 arithmetic.
// fp32 operation order (the build has -ffp-contract=off; / and sqrtf are correctly rounded), for a triplet (i, j, k):
//   e1 = a_j - a_i, e2 = a_k - a_i, n = e1 x e2 with (e1 x e2)_x = e1_y e2_z - e1_z e2_y (cyclic); |v|^2 = (v_x^2 + v_y^2) + v_z^2;
//   degenerate when |n|^2 <= (eps_area |e1|^2) |e2|^2;  u1 = e1 / sqrt(|e1|^2), u3 = n / sqrt(|n|^2), u2 = u3 x u1;  v1, v2, v3 from b alike;
//   R_rc = (v1_r u1_c + v2_r u2_c) + v3_r u3_c;  t_r = b_i,r - ((R_r0 a_i,x + R_r1 a_i,y) + R_r2 a_i,z);
//   q_r = ((R_r0 a_x + R_r1 a_y) + R_r2 a_z) + t_r;  d^2 = ((q_x - b_x)^2 + (q_y - b_y)^2) + (q_z - b_z)^2;  inlier iff d^2 <= thresh * thresh.
#include "common.h"

constexpr int RS_LANES = 64;          // hypotheses per workgroup (one wave) and rows per LDS tile
constexpr int RS_ROW = 8;             // floats per staged row: a_x a_y a_z 0 b_x b_y b_z 0
constexpr int RS_TARGET_WG = 2048;    // workgroups asked for (8 per CU): slices are added until the grid reaches it ...
constexpr int RS_MIN_SLICE = 128;     // ... but no slice is shorter than this many correspondences
constexpr int RS_SELECT_BLOCK = 1024;
constexpr int RS_INLIER_BLOCK = 1024;

struct RsPose { float r00, r01, r02, r10, r11, r12, r20, r21, r22, t0, t1, t2; };

// slices of the correspondences and rows per slice: a function of H and N only
static inline void rs_slices(int N, int H, int* S, int* len)
{
    const int G = (H + RS_LANES - 1) / RS_LANES;
    int s = (RS_TARGET_WG + G - 1) / G;
    const int smax = (N + RS_MIN_SLICE - 1) / RS_MIN_SLICE;
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    const int l = N > 0 ? (N + s - 1) / s : 1;
    *len = l;
    *S = N > 0 ? (N + l - 1) / l : 1;
}

__device__ __forceinline__ float rs_norm2(float x, float y, float z) { return (x * x + y * y) + z * z; }

// unit frame (u1, u2, u3) of the legs e1 = p_j - p_i, e2 = p_k - p_i; false when the triangle is degenerate
__device__ __forceinline__ bool rs_frame(const float* __restrict__ p, int i, int j, int k, float eps_area, float (&u)[9])
{
    const float pi0 = p[(size_t)i * 3], pi1 = p[(size_t)i * 3 + 1], pi2 = p[(size_t)i * 3 + 2];
    const float e10 = p[(size_t)j * 3] - pi0, e11 = p[(size_t)j * 3 + 1] - pi1, e12 = p[(size_t)j * 3 + 2] - pi2;
    const float e20 = p[(size_t)k * 3] - pi0, e21 = p[(size_t)k * 3 + 1] - pi1, e22 = p[(size_t)k * 3 + 2] - pi2;
    const float n0 = e11 * e22 - e12 * e21, n1 = e12 * e20 - e10 * e22, n2 = e10 * e21 - e11 * e20;
    const float l1 = rs_norm2(e10, e11, e12), l2 = rs_norm2(e20, e21, e22), ln = rs_norm2(n0, n1, n2);
    if (!(ln > (eps_area * l1) * l2)) return false;          // also a NaN or a zero leg
    const float s1 = sqrtf(l1), sn = sqrtf(ln);
    u[0] = e10 / s1; u[1] = e11 / s1; u[2] = e12 / s1;
    u[6] = n0 / sn; u[7] = n1 / sn; u[8] = n2 / sn;
    u[3] = u[7] * u[2] - u[8] * u[1]; u[4] = u[8] * u[0] - u[6] * u[2]; u[5] = u[6] * u[1] - u[7] * u[0];
    return true;
}

// the minimal solver: (R, t) of the triplet, false for an invalid hypothesis
__device__ __forceinline__ bool rs_triad(const float* __restrict__ a, const float* __restrict__ b, int N, int i, int j, int k, float eps_area, RsPose& P)
{
    if (i < 0 || j < 0 || k < 0 || i >= N || j >= N || k >= N || i == j || i == k || j == k) return false;
    float u[9], v[9];
    if (!rs_frame(a, i, j, k, eps_area, u)) return false;
    if (!rs_frame(b, i, j, k, eps_area, v)) return false;
    P.r00 = (v[0] * u[0] + v[3] * u[3]) + v[6] * u[6]; P.r01 = (v[0] * u[1] + v[3] * u[4]) + v[6] * u[7]; P.r02 = (v[0] * u[2] + v[3] * u[5]) + v[6] * u[8];
    P.r10 = (v[1] * u[0] + v[4] * u[3]) + v[7] * u[6]; P.r11 = (v[1] * u[1] + v[4] * u[4]) + v[7] * u[7]; P.r12 = (v[1] * u[2] + v[4] * u[5]) + v[7] * u[8];
    P.r20 = (v[2] * u[0] + v[5] * u[3]) + v[8] * u[6]; P.r21 = (v[2] * u[1] + v[5] * u[4]) + v[8] * u[7]; P.r22 = (v[2] * u[2] + v[5] * u[5]) + v[8] * u[8];
    const float a0 = a[(size_t)i * 3], a1 = a[(size_t)i * 3 + 1], a2 = a[(size_t)i * 3 + 2];
    P.t0 = b[(size_t)i * 3] - ((P.r00 * a0 + P.r01 * a1) + P.r02 * a2);
    P.t1 = b[(size_t)i * 3 + 1] - ((P.r10 * a0 + P.r11 * a1) + P.r12 * a2);
    P.t2 = b[(size_t)i * 3 + 2] - ((P.r20 * a0 + P.r21 * a1) + P.r22 * a2);
    return true;
}

__device__ __forceinline__ float rs_d2(const RsPose& P, float ax, float ay, float az, float bx, float by, float bz)
{
    const float q0 = ((P.r00 * ax + P.r01 * ay) + P.r02 * az) + P.t0;
    const float q1 = ((P.r10 * ax + P.r11 * ay) + P.r12 * az) + P.t1;
    const float q2 = ((P.r20 * ax + P.r21 * ay) + P.r22 * az) + P.t2;
    const float r0 = q0 - bx, r1 = q1 - by, r2 = q2 - bz;
    return (r0 * r0 + r1 * r1) + r2 * r2;
}

__global__ __launch_bounds__(RS_LANES) void ransac_score_kernel(const float* __restrict__ a, const float* __restrict__ b, int N, const int* __restrict__ trip, int H,
                                                                float th2, float eps_area, int slice_len, int* __restrict__ cells)
{
    __shared__ f32x4_t rows[RS_LANES * 2];
    const int lane = threadIdx.x;
    const int h = (int)blockIdx.x * RS_LANES + lane;
    RsPose P = {};
    bool valid = false;
    if (h < H) valid = rs_triad(a, b, N, trip[(size_t)h * 3], trip[(size_t)h * 3 + 1], trip[(size_t)h * 3 + 2], eps_area, P);
    const int c0 = (int)blockIdx.y * slice_len, c1 = min(c0 + slice_len, N);
    int count = 0;
    // the next tile's row of this lane waits in registers while the current tile is scored
    float na[3] = {0.f, 0.f, 0.f}, nb[3] = {0.f, 0.f, 0.f};
    auto fetch = [&](int base) {
        const int c = base + lane;
        if (c < c1) {
#pragma unroll
            for (int d = 0; d < 3; ++d) { na[d] = a[(size_t)c * 3 + d]; nb[d] = b[(size_t)c * 3 + d]; }
        }
    };
    fetch(c0);
    for (int base = c0; base < c1; base += RS_LANES) {
        const f32x4_t ra = {na[0], na[1], na[2], 0.f}, rb = {nb[0], nb[1], nb[2], 0.f};
        __syncthreads();                                     // the previous tile has been read by every lane
        rows[2 * lane] = ra;
        rows[2 * lane + 1] = rb;
        __syncthreads();
        fetch(base + RS_LANES);
        const int n = min(RS_LANES, c1 - base);              // uniform: rows past the slice's end are never read
#pragma unroll 4
        for (int r = 0; r < n; ++r) {
            const f32x4_t pa = rows[2 * r], pb = rows[2 * r + 1];
            count += rs_d2(P, pa.x, pa.y, pa.z, pb.x, pb.y, pb.z) <= th2 ? 1 : 0;
        }
    }
    if (h < H) cells[(size_t)blockIdx.y * H + h] = valid ? count : -1;
}

__global__ __launch_bounds__(RS_SELECT_BLOCK) void ransac_select_kernel(const float* __restrict__ a, const float* __restrict__ b, int N, const int* __restrict__ trip, int H,
                                                                         float eps_area, const int* __restrict__ cells, int S, int* __restrict__ best,
                                                                         float* __restrict__ pose, int* __restrict__ status, int* __restrict__ counts,
                                                                         float* __restrict__ poses)
{
    __shared__ int sScore[RS_SELECT_BLOCK], sIndex[RS_SELECT_BLOCK];
    const int tid = threadIdx.x;
    int bs = -1, bi = 0x7fffffff;
    for (int h = tid; h < H; h += RS_SELECT_BLOCK) {         // ascending h: the strict > keeps the smallest index of this thread's ties
        int score = cells[h];
        if (score >= 0)
            for (int s = 1; s < S; ++s) score += cells[(size_t)s * H + h];
        if (counts) counts[h] = score < 0 ? 0 : score;
        if (poses) {
            RsPose P = {};
            if (score >= 0) rs_triad(a, b, N, trip[(size_t)h * 3], trip[(size_t)h * 3 + 1], trip[(size_t)h * 3 + 2], eps_area, P);
            float* o = poses + (size_t)h * 12;
            o[0] = P.r00; o[1] = P.r01; o[2] = P.r02; o[3] = P.r10; o[4] = P.r11; o[5] = P.r12; o[6] = P.r20; o[7] = P.r21; o[8] = P.r22;
            o[9] = P.t0; o[10] = P.t1; o[11] = P.t2;
        }
        if (score > bs) { bs = score; bi = h; }
    }
    sScore[tid] = bs; sIndex[tid] = bi;
    __syncthreads();
    // (score, index) is a total order, so the tree's shape does not matter: larger score, then smaller index
    for (int o = RS_SELECT_BLOCK / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const int s2 = sScore[tid + o], i2 = sIndex[tid + o];
            if (s2 > sScore[tid] || (s2 == sScore[tid] && i2 < sIndex[tid])) { sScore[tid] = s2; sIndex[tid] = i2; }
        }
        __syncthreads();
    }
    if (tid != 0) return;
    if (sScore[0] < 0) {                                     // no valid hypothesis: the pose buffer is not touched
        best[0] = -1; best[1] = 0; *status = 2;
        return;
    }
    const int h = sIndex[0];
    RsPose P = {};
    rs_triad(a, b, N, trip[(size_t)h * 3], trip[(size_t)h * 3 + 1], trip[(size_t)h * 3 + 2], eps_area, P);
    pose[0] = P.r00; pose[1] = P.r01; pose[2] = P.r02; pose[3] = P.r10; pose[4] = P.r11; pose[5] = P.r12; pose[6] = P.r20; pose[7] = P.r21; pose[8] = P.r22;
    pose[9] = P.t0; pose[10] = P.t1; pose[11] = P.t2;
    best[0] = h; best[1] = sScore[0]; *status = 0;
}

// gate (optional): a status word on the device; non-zero means "no pose": the mask is cleared and the count is 0
__global__ __launch_bounds__(RS_INLIER_BLOCK) void pose_inliers_kernel(const float* __restrict__ a, const float* __restrict__ b, int N, const float* __restrict__ pose,
                                                                        float th2, const int* __restrict__ gate, unsigned char* __restrict__ mask, int* __restrict__ count)
{
    __shared__ int sCount[RS_INLIER_BLOCK / 64];
    const int tid = threadIdx.x;
    const bool live = !(gate && *gate != 0);
    RsPose P = {};
    if (live) {
        P.r00 = pose[0]; P.r01 = pose[1]; P.r02 = pose[2]; P.r10 = pose[3]; P.r11 = pose[4]; P.r12 = pose[5]; P.r20 = pose[6]; P.r21 = pose[7]; P.r22 = pose[8];
        P.t0 = pose[9]; P.t1 = pose[10]; P.t2 = pose[11];
    }
    int n = 0;
    for (int c = tid; c < N; c += RS_INLIER_BLOCK) {
        const bool in = live && rs_d2(P, a[(size_t)c * 3], a[(size_t)c * 3 + 1], a[(size_t)c * 3 + 2], b[(size_t)c * 3], b[(size_t)c * 3 + 1], b[(size_t)c * 3 + 2]) <= th2;
        mask[c] = in ? 1 : 0;
        n += in ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((tid & 63) == 0) sCount[tid >> 6] = n;
    __syncthreads();
    if (tid == 0 && count) {
        int t = 0;
        for (int w = 0; w < RS_INLIER_BLOCK / 64; ++w) t += sCount[w];
        *count = t;
    }
}

extern "C" {

// workspace: one int32 cell per (slice, hypothesis)
size_t dreg_pose_ransac_workspace_bytes(int N, int H)
{
    if (N < 0 || H <= 0) return 0;
    int S, len;
    rs_slices(N, H, &S, &len);
    return (size_t)S * (size_t)H * sizeof(int);
}

int dreg_pose_ransac(const float* a, const float* b, int N, const int* triplets, int H, float thresh, float eps_area, void* workspace, size_t workspace_bytes,
                     int* best, float* pose, int* status, int* counts, float* poses, unsigned char* mask, void* stream)
{
    if (N < 0 || H <= 0 || (N > 0 && (!a || !b)) || !triplets || !workspace || !best || !pose || !status) return DREG_EINVAL;
    if (!(thresh >= 0.f) || !(eps_area >= 0.f)) return DREG_EINVAL;
    if (workspace_bytes < dreg_pose_ransac_workspace_bytes(N, H) || ((uintptr_t)workspace & 3)) return DREG_EINVAL;
    int S, len;
    rs_slices(N, H, &S, &len);
    const float th2 = thresh * thresh;
    int* cells = (int*)workspace;
    hipLaunchKernelGGL(ransac_score_kernel, dim3((H + RS_LANES - 1) / RS_LANES, S), dim3(RS_LANES), 0, (hipStream_t)stream, a, b, N, triplets, H, th2, eps_area,
                       len, cells);
    hipLaunchKernelGGL(ransac_select_kernel, dim3(1), dim3(RS_SELECT_BLOCK), 0, (hipStream_t)stream, a, b, N, triplets, H, eps_area, (const int*)cells, S, best,
                       pose, status, counts, poses);
    if (mask && N > 0)
        hipLaunchKernelGGL(pose_inliers_kernel, dim3(1), dim3(RS_INLIER_BLOCK), 0, (hipStream_t)stream, a, b, N, (const float*)pose, th2, (const int*)status, mask,
                           (int*)nullptr);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

int dreg_pose_inliers(const float* a, const float* b, int N, const float* pose, float thresh, unsigned char* mask, int* count, void* stream)
{
    if (N < 0 || (N > 0 && (!a || !b || !mask)) || !pose || !count || !(thresh >= 0.f)) return DREG_EINVAL;
    hipLaunchKernelGGL(pose_inliers_kernel, dim3(1), dim3(RS_INLIER_BLOCK), 0, (hipStream_t)stream, a, b, N, pose, thresh * thresh, (const int*)nullptr, mask, count);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

}  // extern "C"
