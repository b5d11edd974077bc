// The density of a REGISTERED SCENE of K NeRF blocks (1 <= K <= DREG_SCENE_MAX_BLOCKS = 4) as one scalar field, gfx950: the field the K-block
// renderer (render_scene.hip) composites, evaluated at points or over a lattice in ONE kernel, so that the mesher
// (marching_cubes.hip) extracts the surface of the whole registered scene instead of K interleaved ones.  The ONE density-field kernel: the field
// of a registered PAIR (dreg_pair_density; rule: DESIGN.md §3i, CPU restatement: tests/pair_field_restatement.py) is its K = 2 form, a second
// entry point over the same launch (rule: DESIGN.md §3k, CPU restatement: tests/scene_field_restatement.py).
//
// Frames.  The field lives in the SCENE frame (the anchor's frame of pose_graph.synchronize; for a pair the TARGET frame).  Block b has a pose
// G_b = [R_b|t_b] mapping its frame to the scene frame, rounded to fp32 once by the host (12 floats), or no pose.  For a point x (fp32):
//   with a pose     d = x - t_b, x_b[k] = (R_b[0][k] d[0] + R_b[1][k] d[1]) + R_b[2][k] d[2]    (fp32, this order, no contraction: the same bits
//                   as torch fp32 elementwise ops)
//   without         x_b = x, the same bits
// Own coverage     m_b(x_b): march_covered (inside the roi, the cell clamp(floor(u res), 0, res - 1) set): a block contributes only where its OWN
//                  occupancy cell is set (the renderer marches only occupied cells; floaters outside the grids are gone)
// Densities        sigma_b = block b's density at x_b, the dense query's bit for bit (ngp_unit_cube, ngp_level_features, ngp_density_mlp,
//                  __expf(h0 - 1) times the strictly-inside flag)
// Weight           render_scene.hip's overlap weight, operation for operation: delta_b = |x_b - c_b|^2 + 1e-12f (the squares summed from 0.f in axis
//                  order), C_b = the OTHER blocks with m = 1;  m_b = 0: omega_b = 0;  |C_b| = 0: omega_b = 1;
//                  |C_b| = 1: with lo / hi the lower / higher index of the two, omega_lo = 1 / (1 + __expf(p/2 __logf(delta_lo / delta_hi))),
//                             omega_hi = 1 - omega_lo;
//                  |C_b| >= 2: omega_b = 1 / (1 + sum over b' in C_b, ascending, of __expf(p/2 __logf(delta_b / delta_b')))
// Scene density    sigma = ((p_0 + p_1) + p_2) + p_3 with p_b = fl(omega_b sigma_b); absent or uncovered blocks contribute + 0.f (every term is >= 0:
//                  adding + 0.f changes no bit).  Where one block alone covers the point sigma is that block's sigma exactly.
// The pair         K = 2, blocks [(src, P), (tgt, none)]: w_S = omega_0 = m_S ? (m_T ? w : 1) : 0 with w = 1 / (1 + __expf(p/2 __logf(delta_S /
//                  delta_T))), w_T = omega_1 = m_T ? (m_S ? 1 - w : 1) : 0, sigma_P = fl(fl(w_S sigma_S) + fl(w_T sigma_T)).
//
// One lane = one point, 64 points per wave, one-wave workgroups that stride over the 64-point chunks (ngp_density_kernel's shape).  Points form:
// chunk c holds points 64 c .. 64 c + 63 of x [N,3].  Lattice form: lanes run along x — a chunk is 64 x-contiguous nodes of one (y,z) row, the
// lane forms its node's position origin_c + (float)i_c * spacing_c itself (the position dreg_mc_emit gives the node), output [nz,ny,nx]; no
// position tensor exists.  Per chunk: the positions and all K coverages (a bit mask per lane) and distances, then the weights, then block b's
// density phase (its MFMA operands, the 16-level gather, the MLP through the one 64 x 64 fp16 LDS tile) only when some lane has m_b set, so a
// chunk outside every grid costs the K lookups and a store.  Every loop over the block index that reads a block is ONE non-unrolled body that
// reads the block and its pose from the kernel-argument segment, for the reason render_pair.hip's header gives.  Nothing per-lane is indexed by
// a run-time block index (that would go to scratch): delta_b, sigma_b and omega_b sit in K named registers, written by select inside unrolled
// loops, and x_b is recomputed in the phase from the same operands (the same bits).  The per-block parts go out through one nullable pointer per
// block and array and one stride: [n,K] rows for the scene entry, four separate [n] arrays for the pair entry.  No atomics, no process-global
// state; a point's result depends on nothing but the point, so the output is bit-identical between runs, launch widths, orders and forms.  As
// built: DESIGN.md §3k.
#include "scene_field.h"   // SceneFieldBlock, its fill, the coverage and the weights: shared with the merged voxel grid (scene_grid.hip)

struct SceneFieldArgs {
    SceneFieldBlock b[FIELD_MAXB];      // the first K are filled, the rest zero
    int K;
    float half_power;
    const float* x;             // points form: [n,3]; null: lattice form
    float origin[3], spacing[3];
    int nx, ny;                 // lattice form: nodes per x row, rows per z plane
    int chunks_per_row;         // lattice form: ceil(nx / 64)
    long n;                     // points, or nodes (nx ny nz)
    long chunks;                // 64-point chunks of the launch
    float* sigma;               // [n]
    float *weight_out[FIELD_MAXB], *sigma_out[FIELD_MAXB];     // block j's omega_j / sigma_j of point i at [i * part_stride]; each may be null
    long part_stride;
};
static_assert(sizeof(SceneFieldArgs) <= 4096, "the blocks are read from the kernel-argument segment");

static constexpr long SCENE_FIELD_WAVES = 16384;    // one-wave workgroups of the launch at most (256 CUs x 16 resident x 4 rounds)

// four waves per SIMD, the residency the 9.25 KB of LDS per wave admit (16 workgroups per CU): without the attribute the two-block form of this
// kernel took 79 VGPRs + 64 AGPRs, three waves per SIMD; the gathers of a phase are latency, which occupancy hides
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void scene_density_kernel(SceneFieldArgs a)
{
    // ONE 64 x 64 fp16 tile per wave, the encoded input in its first rows until the first layer has read it (ngp_density_kernel's layout:
    // allowed by ngp_density_mlp, the epilogue below writes sOut only)
    __shared__ __attribute__((aligned(16))) char sH[64 * NGP_HRS];
    __shared__ float sOut[64];
    char* sX = sH;
    const int lane = threadIdx.x;
    const int fr = lane & 15, kg = lane >> 4;
    const int K = a.K;
    for (long chunk = blockIdx.x; chunk < a.chunks; chunk += gridDim.x) {
        // ---- the lane's point in the scene frame and where its results go
        long idx;
        bool valid;
        float xw[3] = {0.f, 0.f, 0.f};
        if (a.x != nullptr) {
            idx = chunk * 64 + lane;
            valid = idx < a.n;
            if (valid) {
#pragma unroll
                for (int k = 0; k < 3; ++k) xw[k] = a.x[idx * 3 + k];
            }
        } else {
            const long row = chunk / a.chunks_per_row;                    // iy + ny * iz
            const int ix = (int)(chunk - row * a.chunks_per_row) * 64 + lane;
            const int iz = (int)(row / a.ny), iy = (int)(row - (long)iz * a.ny);
            valid = ix < a.nx;
            idx = row * a.nx + ix;
            const int ic[3] = {ix, iy, iz};
#pragma unroll
            for (int k = 0; k < 3; ++k) xw[k] = a.origin[k] + (float)ic[k] * a.spacing[k];
        }
        // ---- every block's own coverage (a bit per block), the point's squared distance to the block's camera centroid, the overlap weights
        unsigned mask;
        float del[FIELD_MAXB], om[FIELD_MAXB];
        scene_field_coverage(a.b, K, valid, xw, mask, del);
        scene_field_weights(mask, del, a.half_power, om);
        // ---- each block's density where that block covers the point; one body serves all blocks (the block's arguments are read per phase)
        float sig[FIELD_MAXB] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int q = 0; q < K; ++q) {
            const bool have = (mask >> q) & 1u;
            if (!__any(have)) continue;
            // (the phase is ALSO stated as scene_field_density in scene_field.h, which scene_grid.hip calls; this kernel keeps its body written
            // out: through the function it took 119 instead of 117 VGPRs.  tests/test_hip_scene_grid.py holds the two to the same bits.)
            const SceneFieldBlock& b = a.b[q];
            float xb[3], u[3];
            scene_field_to_block(b, xw, xb);
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
#pragma unroll
            for (int j = 0; j < FIELD_MAXB; ++j) sig[j] = (j == q && have) ? s : sig[j];
            wave_sync();                                                             // sOut and the tile are rewritten by the next phase
        }
        if (valid) {
            a.sigma[idx] = ((om[0] * sig[0] + om[1] * sig[1]) + om[2] * sig[2]) + om[3] * sig[3];
#pragma unroll
            for (int j = 0; j < FIELD_MAXB; ++j) {           // (the pointers of blocks >= K are null)
                if (a.weight_out[j]) a.weight_out[j][idx * a.part_stride] = om[j];
                if (a.sigma_out[j]) a.sigma_out[j][idx * a.part_stride] = sig[j];
            }
        }
    }
}

// The ONE launch behind both entry points, and the one statement of the forms, the lattice limits, the chunk counts and the launch width.
// weight_out / sigma_out: n_blocks pointers each (any may be null: not written), block j's value of point i at [i * part_stride].
static int scene_density_launch(const float* x, long n, const float* origin, const float* spacing, int nx, int ny, int nz, int n_blocks,
                                const dreg_field_block* blocks, float power, float* sigma, float* const* weight_out, float* const* sigma_out,
                                long part_stride, void* stream)
{
    const bool lattice = origin != nullptr || spacing != nullptr;
    if (n < 0 || !(power > 0.f) || !(power <= 3.0e38f)) return DREG_EINVAL;
    if (lattice) {
        if (x || !origin || !spacing) return DREG_EINVAL;
        if (nx < 2 || ny < 2 || nz < 2 || nx > 1024 || ny > 1024 || nz > 1024 || (long)nx * ny * nz > (1l << 28)) return DREG_EINVAL;
    } else if (n == 0) return DREG_OK;
    if ((!lattice && !x) || !sigma) return DREG_EINVAL;
    SceneFieldArgs a;
    __builtin_memset(&a, 0, sizeof(a));
    for (int b = 0; b < n_blocks; ++b)
        if (scene_field_fill(a.b[b], blocks[b]) != DREG_OK) return DREG_EINVAL;
    a.K = n_blocks;
    for (int k = 0; k < 3; ++k) { a.origin[k] = lattice ? origin[k] : 0.f; a.spacing[k] = lattice ? spacing[k] : 0.f; }
    a.half_power = 0.5f * power;
    a.x = x;
    a.nx = lattice ? nx : 0; a.ny = lattice ? ny : 1;
    a.chunks_per_row = lattice ? (nx + 63) / 64 : 1;
    a.n = lattice ? (long)nx * ny * nz : n;
    a.chunks = lattice ? (long)a.chunks_per_row * ny * nz : (n + 63) / 64;
    a.sigma = sigma;
    for (int b = 0; b < n_blocks; ++b) { a.weight_out[b] = weight_out[b]; a.sigma_out[b] = sigma_out[b]; }
    a.part_stride = part_stride;
    const long waves = a.chunks < SCENE_FIELD_WAVES ? a.chunks : SCENE_FIELD_WAVES;
    hipLaunchKernelGGL(scene_density_kernel, dim3((unsigned)waves), dim3(64), 0, (hipStream_t)stream, a);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

extern "C" {

// The scene density of n_blocks blocks (HOST array `blocks`) at n points or at the nodes of a lattice; see include/dreg_nerf.h.
int dreg_scene_density(const float* x, long n, const float* origin, const float* spacing, int nx, int ny, int nz, int n_blocks,
                       const dreg_field_block* blocks, float power, float* sigma, float* weight_block, float* sigma_block, void* stream)
{
    if (n_blocks < 1 || n_blocks > FIELD_MAXB || !blocks) return DREG_EINVAL;
    float *w[FIELD_MAXB], *s[FIELD_MAXB];                    // [n,K] rows: block j's column
    for (int j = 0; j < n_blocks; ++j) { w[j] = weight_block ? weight_block + j : nullptr; s[j] = sigma_block ? sigma_block + j : nullptr; }
    return scene_density_launch(x, n, origin, spacing, nx, ny, nz, n_blocks, blocks, power, sigma, w, s, n_blocks, stream);
}

// The pair density: the K = 2 form, blocks {(src, pose), (tgt, none)}, the parts in four separate [n] arrays; see include/dreg_nerf.h.
int dreg_pair_density(const float* x, long n, const float* origin, const float* spacing, int nx, int ny, int nz,
                      const uint8_t* src_binary, int src_rx, int src_ry, int src_rz, const void* src_table, const void* src_w1, const void* src_w2,
                      const uint32_t* src_offset, const uint32_t* src_size, const uint32_t* src_res, const float* src_scale, const uint32_t* src_hashed,
                      const float* src_roi_aabb, const float* src_model_aabb, const float* src_center,
                      const uint8_t* tgt_binary, int tgt_rx, int tgt_ry, int tgt_rz, const void* tgt_table, const void* tgt_w1, const void* tgt_w2,
                      const uint32_t* tgt_offset, const uint32_t* tgt_size, const uint32_t* tgt_res, const float* tgt_scale, const uint32_t* tgt_hashed,
                      const float* tgt_roi_aabb, const float* tgt_model_aabb, const float* tgt_center,
                      const float* pose, float power, float* sigma, float* w_src, float* w_tgt, float* sigma_src, float* sigma_tgt, void* stream)
{
    // the source block must have a pose (the scene entry takes a block without one); points form with n == 0 stays DREG_OK before any null check
    if (!pose && (origin || spacing || n != 0)) return DREG_EINVAL;
    const dreg_field_block blocks[2] = {
        {src_binary, src_rx, src_ry, src_rz, src_table, src_w1, src_w2, src_offset, src_size, src_res, src_scale, src_hashed, src_roi_aabb, src_model_aabb,
         src_center, pose},
        {tgt_binary, tgt_rx, tgt_ry, tgt_rz, tgt_table, tgt_w1, tgt_w2, tgt_offset, tgt_size, tgt_res, tgt_scale, tgt_hashed, tgt_roi_aabb, tgt_model_aabb,
         tgt_center, nullptr}};
    float* const w[2] = {w_src, w_tgt};
    float* const s[2] = {sigma_src, sigma_tgt};
    return scene_density_launch(x, n, origin, spacing, nx, ny, nz, 2, blocks, power, sigma, w, s, 1, stream);
}

}  // extern "C"
