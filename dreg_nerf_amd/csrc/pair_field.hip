// The density of a REGISTERED PAIR of NeRF blocks as one scalar field, gfx950: the field the two-block renderer (render_pair.hip, DESIGN.md
// §3e) composites, evaluated at points or over a lattice in ONE kernel, so that the mesher (marching_cubes.hip) extracts the surface of the
// merged scene instead of two interleaved ones (rule: DESIGN.md §3i, CPU restatement: tests/pair_field_restatement.py).
//
// Frames.  The pose P = [R|t] maps the source frame to the target frame; the field lives in the TARGET frame.  The host rounds the fp64 pose to
// fp32 once (Rf row-major, tf) and the kernel receives those 12 floats.  For a point x (fp32): x_T = x, d = x - tf,
//   x_S[k] = (Rf[0][k] d[0] + Rf[1][k] d[1]) + Rf[2][k] d[2]       (fp32, this order, no contraction: the same bits as torch fp32 elementwise ops)
// Own coverage     m_b(x_b): x_b lies in block b's occupancy roi (u = (x - lo) / ext, 0 <= u <= 1 on all axes) and the cell
//                  clamp(floor(u res), 0, res - 1) is set — pair_covered's lookup of render_pair.hip without the ray-interval clause
// Densities        sigma_b = block b's density at x_b, the dense query's bit for bit (ngp_unit_cube, ngp_level_features, ngp_density_mlp,
//                  __expf(h0 - 1) times the strictly-inside flag), each block with its own aabb, levels, table and weights
// Weight           q = (|x_S - c_S|^2 + 1e-12) / (|x_T - c_T|^2 + 1e-12), w = 1 / (1 + __expf(0.5 p __logf(q))): render_pair.hip's, operation
//                  for operation (c_b: the centroid of block b's cameras in its own frame)
// Pair density     w_S = m_S ? (m_T ? w : 1) : 0,  w_T = m_T ? (m_S ? 1 - w : 1) : 0,  sigma_P = fl(fl(w_S sigma_S) + fl(w_T sigma_T)):
//                  a block contributes only where its OWN occupancy cell is set (the renderer marches only occupied cells; floaters
//                  outside the grids are gone), and where one block alone is present sigma_P is that block's sigma exactly.
//
// One lane = one point, 64 points per wave, one-wave workgroups that stride over the 64-point chunks (ngp_density_kernel's shape).  Points
// form: chunk c holds points 64 c .. 64 c + 63 of x [N,3].  Lattice form: lanes run along x — a chunk is 64 x-contiguous nodes of one (y,z)
// row, the lane forms its node's position origin_c + (float)i_c * spacing_c itself (the position dreg_mc_emit gives the node), output
// [nz,ny,nx]; no position tensor exists.  Per chunk the positions and both coverages come first; a block's phase (its MFMA operands, the
// 16-level gather, the MLP, sigma) runs only when some lane has m_b set, so a chunk outside both grids costs the two lookups and a store.
// The two phases are ONE loop body over the block index (not unrolled) that reads the block from the kernel-argument segment, for the reason
// render_pair.hip's header gives.  No atomics, no process-global state; a point's result depends on nothing but the point, so the output
// is bit-identical between runs, launch widths, orders and forms.  As built: DESIGN.md §3i.
#include "march.h"
#include "../../include/dreg_nerf.h"   // signature check of the entry point defined here

struct PairFieldBlock : MarchBlock {
    float center[3];            // centroid of the block's cameras, in the block's frame
};

struct PairFieldArgs {
    PairFieldBlock b[2];        // 0 = source, 1 = target
    float R[9], t[3];           // the pose rounded to fp32: R row-major, then t
    float half_power;
    const float* x;             // points form: [n,3]; null: lattice form
    float origin[3], spacing[3];
    int nx, ny;                 // lattice form: nodes per x row, rows per z plane
    int chunks_per_row;         // lattice form: ceil(nx / 64)
    long n;                     // points, or nodes (nx ny nz)
    long chunks;                // 64-point chunks of the launch
    float *sigma, *w_src, *w_tgt, *sigma_src, *sigma_tgt;      // the last four may be null
};

static constexpr long PAIR_FIELD_WAVES = 16384;     // one-wave workgroups of the launch at most (256 CUs x 16 resident x 4 rounds)

// whether block b's own occupancy grid covers the point x of its frame: inside the roi, in a set cell (pair_covered without the ray interval)
__device__ __forceinline__ bool pair_field_covered(const MarchBlock& b, const float (&x)[3])
{
    const int rdim[3] = {b.rx, b.ry, b.rz};
    float u[3];
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) { u[k] = (x[k] - b.roi[k]) / (b.roi[3 + k] - b.roi[k]); inside = inside && u[k] >= 0.f && u[k] <= 1.f; }
    if (!inside) return false;
    int ci[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ci[k] = min(max((int)floorf(u[k] * (float)rdim[k]), 0), rdim[k] - 1);
    return b.binary[((long)ci[0] * b.ry + ci[1]) * b.rz + ci[2]] != 0;
}

// four waves per SIMD, the residency the 9.25 KB of LDS per wave admit (16 workgroups per CU): without the attribute the kernel took 79 VGPRs + 64
// AGPRs, three waves per SIMD; the gathers of a phase are latency, which occupancy hides
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void pair_density_kernel(PairFieldArgs a)
{
    // ONE 64 x 64 fp16 tile per wave, the encoded input in its first rows until the first layer has read it (ngp_density_kernel's layout:
    // allowed by ngp_density_mlp, the epilogue below writes sOut only)
    __shared__ __attribute__((aligned(16))) char sH[64 * NGP_HRS];
    __shared__ float sOut[64];
    char* sX = sH;
    const int lane = threadIdx.x;
    const int fr = lane & 15, kg = lane >> 4;
    for (long chunk = blockIdx.x; chunk < a.chunks; chunk += gridDim.x) {
        // ---- the lane's point in the target frame and where its results go
        long idx;
        bool valid;
        float xt[3] = {0.f, 0.f, 0.f};
        if (a.x != nullptr) {
            idx = chunk * 64 + lane;
            valid = idx < a.n;
            if (valid) {
#pragma unroll
                for (int k = 0; k < 3; ++k) xt[k] = a.x[idx * 3 + k];
            }
        } else {
            const long row = chunk / a.chunks_per_row;                    // iy + ny * iz
            const int ix = (int)(chunk - row * a.chunks_per_row) * 64 + lane;
            const int iz = (int)(row / a.ny), iy = (int)(row - (long)iz * a.ny);
            valid = ix < a.nx;
            idx = row * a.nx + ix;
            const int ic[3] = {ix, iy, iz};
#pragma unroll
            for (int k = 0; k < 3; ++k) xt[k] = a.origin[k] + (float)ic[k] * a.spacing[k];
        }
        // ---- the same point in the source frame: x_S = R^T (x - t)
        float xs[3];
        {
            const float d[3] = {xt[0] - a.t[0], xt[1] - a.t[1], xt[2] - a.t[2]};
#pragma unroll
            for (int k = 0; k < 3; ++k) xs[k] = (a.R[k] * d[0] + a.R[3 + k] * d[1]) + a.R[6 + k] * d[2];
        }
        // ---- own coverage, then the overlap weight where both blocks cover the point (render_pair.hip's arithmetic)
        const bool m_s = valid && pair_field_covered(a.b[0], xs);
        const bool m_t = valid && pair_field_covered(a.b[1], xt);
        float w_s = m_s ? 1.f : 0.f, w_t = m_t ? 1.f : 0.f;
        if (m_s && m_t) {
            float ds = 0.f, dt2 = 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float es = xs[k] - a.b[0].center[k], et = xt[k] - a.b[1].center[k];
                ds += es * es; dt2 += et * et;
            }
            const float q = (ds + 1e-12f) / (dt2 + 1e-12f);
            w_s = 1.f / (1.f + __expf(a.half_power * __logf(q)));                 // 1 / (1 + q^(p/2))
            w_t = 1.f - w_s;
        }
        // ---- each block's density where that block covers the point; one body serves both blocks (the block's arguments are read per phase)
        float sig[2] = {0.f, 0.f};
#pragma unroll 1
        for (int q = 0; q < 2; ++q) {
            const bool have = q == 0 ? m_s : m_t;
            if (!__any(have)) continue;
            const PairFieldBlock& b = a.b[q];
            float xb[3], u[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) xb[k] = q == 0 ? xs[k] : xt[k];
            const bool inside_m = ngp_unit_cube(xb, b.model, b.model + 3, 0, u);
#pragma unroll 1
            for (int l = 0; l < 16; ++l) {
                float f0 = 0.f, f1 = 0.f;
                if (have) ngp_level_features(b.table, b.lv, l, u, f0, f1);
                _Float16* xr = reinterpret_cast<_Float16*>(sX + lane * NGP_XRS);
                xr[2 * l] = (_Float16)f0; xr[2 * l + 1] = (_Float16)f1;
            }
            NgpDensityW dw;
            ngp_load_density_w(dw, b.w1, b.w2, lane);
            ngp_density_mlp(dw, sX, sH, lane, [&](int rb, const f32x4_t& ov) {      // ov[r] = output fr of point rb*16 + kg*4 + r
                if (fr == 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) sOut[rb * 16 + kg * 4 + r] = (float)(_Float16)ov[r];
                }
            });
            wave_sync();
            const float s = __expf(sOut[lane] - 1.f) * (inside_m ? 1.f : 0.f);          // the dense query's density (ngp_density_kernel)
            if (have) { if (q == 0) sig[0] = s; else sig[1] = s; }
            wave_sync();                                                             // sOut and the tile are rewritten by the next phase
        }
        if (valid) {
            const float ps = w_s * sig[0], pt = w_t * sig[1];
            a.sigma[idx] = ps + pt;
            if (a.w_src) a.w_src[idx] = w_s;
            if (a.w_tgt) a.w_tgt[idx] = w_t;
            if (a.sigma_src) a.sigma_src[idx] = sig[0];
            if (a.sigma_tgt) a.sigma_tgt[idx] = sig[1];
        }
    }
}

// One block's arguments: its occupancy grid over the roi, its density net and its camera centroid.
struct PairFieldBlockHost {
    const uint8_t* binary;
    int rx, ry, rz;
    const void *table, *w1, *w2;
    const uint32_t *offset, *size, *res;
    const float* scale;
    const uint32_t* hashed;
    const float *roi_aabb, *model_aabb, *center;
};

static int pair_field_fill(PairFieldBlock& b, const PairFieldBlockHost& h)
{
    if (!h.center) return DREG_EINVAL;
    for (int k = 0; k < 3; ++k) b.center[k] = h.center[k];
    // no ray is marched: no colour net, no scene interval (the roi stands in for the scene aabb, the step for a positive number)
    return march_fill_block(b, h.binary, h.rx, h.ry, h.rz, nullptr, h.table, h.w1, h.w2, false, nullptr, nullptr, nullptr, h.offset, h.size, h.res, h.scale,
                            h.hashed, h.roi_aabb, h.roi_aabb, h.model_aabb, 0.f, 0.f, 1.f, 0.f, false);
}

static int pair_density_launch(const float* x, long n, const float* origin, const float* spacing, int nx, int ny, int nz, const PairFieldBlockHost& src,
                               const PairFieldBlockHost& tgt, const float* pose, float power, float* sigma, float* w_src, float* w_tgt, float* sigma_src,
                               float* sigma_tgt, void* stream)
{
    const bool lattice = origin != nullptr || spacing != nullptr;
    if (n < 0 || !(power > 0.f) || !(power <= 3.0e38f)) return DREG_EINVAL;
    if (lattice) {
        if (x || !origin || !spacing) return DREG_EINVAL;
        if (nx < 2 || ny < 2 || nz < 2 || nx > 1024 || ny > 1024 || nz > 1024 || (long)nx * ny * nz > (1l << 28)) return DREG_EINVAL;
    } else if (n == 0) return DREG_OK;
    if ((!lattice && !x) || !pose || !sigma) return DREG_EINVAL;
    PairFieldArgs a;
    if (pair_field_fill(a.b[0], src) != DREG_OK || pair_field_fill(a.b[1], tgt) != DREG_OK) return DREG_EINVAL;
    for (int k = 0; k < 9; ++k) a.R[k] = pose[k];
    for (int k = 0; k < 3; ++k) { a.t[k] = pose[9 + k]; a.origin[k] = lattice ? origin[k] : 0.f; a.spacing[k] = lattice ? spacing[k] : 0.f; }
    a.half_power = 0.5f * power;
    a.x = x;
    a.nx = lattice ? nx : 0; a.ny = lattice ? ny : 1;
    a.chunks_per_row = lattice ? (nx + 63) / 64 : 1;
    a.n = lattice ? (long)nx * ny * nz : n;
    a.chunks = lattice ? (long)a.chunks_per_row * ny * nz : (n + 63) / 64;
    a.sigma = sigma; a.w_src = w_src; a.w_tgt = w_tgt; a.sigma_src = sigma_src; a.sigma_tgt = sigma_tgt;
    const long waves = a.chunks < PAIR_FIELD_WAVES ? a.chunks : PAIR_FIELD_WAVES;
    hipLaunchKernelGGL(pair_density_kernel, dim3((unsigned)waves), dim3(64), 0, (hipStream_t)stream, a);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

extern "C" {

// The pair density at n points x fp32 [n,3] (points form: origin = spacing = null) or at the nodes of a lattice (lattice form: x = null, n ignored;
// origin, spacing: 3 fp32 each in HOST memory; node (ix,iy,iz) at origin[c] + (float)i_c * spacing[c]; outputs [nz,ny,nx], x fastest).  Points
// are in the TARGET frame.  Per block (src_*, tgt_*): binary uint8 [rx,ry,rz] over roi_aabb, the density net and level arrays as
// dreg_ngp_density_fwd takes them, model_aabb and center (the block's camera centroid in its own frame) — aabbs, level arrays and centers in
// HOST memory.  pose: 12 fp32 in HOST memory, R row-major then t, source -> target.  Outputs on the device: sigma fp32 [n]; optional (null =
// not written) w_src, w_tgt, sigma_src, sigma_tgt fp32 [n].  One launch on `stream`; never allocates.
int dreg_pair_density(const float* x, long n, const float* origin, const float* spacing, int nx, int ny, int nz,
                      const uint8_t* src_binary, int src_rx, int src_ry, int src_rz, const void* src_table, const void* src_w1, const void* src_w2,
                      const uint32_t* src_offset, const uint32_t* src_size, const uint32_t* src_res, const float* src_scale, const uint32_t* src_hashed,
                      const float* src_roi_aabb, const float* src_model_aabb, const float* src_center,
                      const uint8_t* tgt_binary, int tgt_rx, int tgt_ry, int tgt_rz, const void* tgt_table, const void* tgt_w1, const void* tgt_w2,
                      const uint32_t* tgt_offset, const uint32_t* tgt_size, const uint32_t* tgt_res, const float* tgt_scale, const uint32_t* tgt_hashed,
                      const float* tgt_roi_aabb, const float* tgt_model_aabb, const float* tgt_center,
                      const float* pose, float power, float* sigma, float* w_src, float* w_tgt, float* sigma_src, float* sigma_tgt, void* stream)
{
    const PairFieldBlockHost src = {src_binary, src_rx, src_ry, src_rz, src_table, src_w1, src_w2, src_offset, src_size, src_res, src_scale, src_hashed,
                                    src_roi_aabb, src_model_aabb, src_center};
    const PairFieldBlockHost tgt = {tgt_binary, tgt_rx, tgt_ry, tgt_rz, tgt_table, tgt_w1, tgt_w2, tgt_offset, tgt_size, tgt_res, tgt_scale, tgt_hashed,
                                    tgt_roi_aabb, tgt_model_aabb, tgt_center};
    return pair_density_launch(x, n, origin, spacing, nx, ny, nz, src, tgt, pose, power, sigma, w_src, w_tgt, sigma_src, sigma_tgt, stream);
}

}  // extern "C"
