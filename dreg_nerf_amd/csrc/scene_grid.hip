// A REGISTERED SCENE of K NeRF blocks (1 <= K <= DREG_SCENE_MAX_BLOCKS = 4) as ONE voxel grid, gfx950: the extraction of a block (ngp.hip: sample
// positions, dense query, 18-direction mean colour, alpha / keep, the [X,Y,Z,7] grid) for the scene density field of scene_field.hip, in ONE
// kernel.  The result has the format of a block's voxel_grid.pt / voxel_mask.pt, so a registered scene is again an input of the registration
// network.  Rule: DESIGN.md §3l; CPU restatement: tests/scene_grid_restatement.py.
//
// The grid     (rx, ry, rz) cells over the box grid_aabb = (lo | hi) of the scene frame; flat index f = (x ry + y) rz + z (z fastest).
// Sample       u_k = ((float)c_k + j_k) / (float)r_k, w_k = u_k (hi_k - lo_k) + lo_k: grid_sample_points_kernel's fp32 expression, operation for
//              operation; j = the cell's row of the dense jitter [rx ry rz, 3], or 0.5 on every axis without one.
// Per block    x_b, own coverage m_b, delta_b, omega_b, sigma_b as the header of scene_field.hip states them (the functions of scene_field.h: the
//              same code), a_b = fl(omega_b sigma_b), sigma = ((a_0 + a_1) + a_2) + a_3: the bits of dreg_scene_density at w.
// Alpha, keep  alpha = clip(1 - __expf(-delta sigma), 0, 1), keep = sigma > density_thre: ngp_alpha_keep_kernel's arithmetic.
// Colour       of a kept cell: c_b = block b's mean over the 18 fixed directions of the colour net on the 15 features of ITS density phase at
//              x_b (each block in its own frame: ngp_rgb_tile, the per-tile body of ngp_rgb_chunks_kernel: the same sums in the same order);
//              rgb = (sum_b fl(a_b c_b)) / (sum_b a_b), both sums from block 0 upwards in fp32 (a block with a_b = 0 adds + 0.f: no bit
//              changes).  Exactly one block with a_b != 0: rgb = that block's c_b, bit for bit.  The denominator or a product not finite: rgb =
//              c_b of the block with the largest a_b, the lowest index on a tie.  No block with a_b != 0 (possible only with density_thre < 0):
//              rgb = 0.  No NaN reaches the grid (a NaN sigma is not kept).
// Outputs      voxel_grid fp32 [rx ry rz, 7] = (w | rgb | alpha) at kept cells and exactly 0 at all others — the kernel writes every row, there is
//              no separate fill —, keep uint8 [rx ry rz], optional sigma fp32 [rx ry rz].
//
// One lane = one cell, one-wave workgroups that stride over 64-cell chunks (scene_density_kernel's shape).  A wave's lanes run along z, the
// output's fastest axis — a chunk is 64 z-contiguous cells of one (x,y) row, its 64 rows of the grid are 1,792 contiguous bytes.  The other order
// (lanes along x, the fastest axis of the hash tables: ngp.hip measured 807 -> 126 MB of memory-side traffic per block for it in the dense query)
// stays behind a knob of the measurement build (dreg_scene_grid_set_lanes_z(0)): with the scattered 28-byte stores it then takes it measured
// 1.03 to 1.16 times the z order's time on a scene grid, three quarters of whose chunks lie outside every block.
// Per chunk: the samples, all K coverages and distances, the weights, then block b's
// density phase only when some lane has m_b — its 16 fp16 outputs stay in LDS (2 KB per block) —, then sigma, alpha, keep.  The colour net runs
// only if some lane is kept, and for block b only if a kept lane has a_b != 0: those lanes are packed (ballot + rank) into 16-point tiles, the
// 14 weight fragments of the block stay in registers across the tiles and the 18 directions, and a tile's 48 results go back to their lanes
// through LDS.  A point's row of an MFMA tile depends on that row alone, so the packing changes no bit.  Nothing per lane is indexed by a
// run-time block index: a_b sits in four named registers, and the blend keeps running sums (num, den) and the colour of the largest a_b instead of
// K colours.  No atomics; a cell's result depends on that cell only: identical bytes between runs, launch widths and lane orders.
#include "scene_field.h"

static constexpr int SCENE_GRID_NDIR = 18;          // SampleGrid's fixed viewing directions: the rows of a block's dirbias buffer

struct SceneGridArgs {
    SceneFieldBlock b[FIELD_MAXB];      // the first K are filled (cw1 .. cw3 too), the rest zero
    const uint32_t* biaspk[FIELD_MAXB]; // block b's packed direction biases: uint32 [18][64] (the second half of dreg_ngp_dir_bias's buffer)
    int K;
    float half_power;
    int rx, ry, rz;
    int lanes_z;                        // 1 (what ships): a chunk is 64 z-contiguous cells of an (x,y) row; 0: 64 x-contiguous cells of a (y,z) row
    int chunks_per_row;                 // ceil(rx / 64) (lanes_z: ceil(rz / 64))
    long chunks;
    float lo[3], hi[3];
    const float* jitter;                // [rx ry rz, 3] or null (0.5)
    float delta, thre;
    float* grid;                        // [rx ry rz, 7]
    uint8_t* keep;                      // [rx ry rz]
    float* sigma;                       // [rx ry rz] or null
};
static_assert(sizeof(SceneGridArgs) <= 4096, "the blocks are read from the kernel-argument segment");

DREG_KNOB(long, g_scene_grid_waves, 16384);     // tuning (include/dreg_nerf_probe.h): one-wave workgroups of the launch at most
DREG_KNOB(int, g_scene_grid_lanes_z, 1);        // tuning (include/dreg_nerf_probe.h): lanes along z (1) or along x (0)

// 18.8 KB of LDS per wave: eight workgroups per CU, two waves per SIMD, which is also what the registers admit
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void scene_grid_kernel(SceneGridArgs a)
{
    __shared__ __attribute__((aligned(16))) char sH[64 * NGP_HRS];              // the density phase's 64 x 64 tile; the colour net's 16 x 64 tile
    __shared__ __attribute__((aligned(16))) _Float16 sF[FIELD_MAXB][64 * 16];   // block b's (h0 | 15 features) of the chunk's 64 cells
    __shared__ __attribute__((aligned(16))) float sC[64 * 4];                   // a block's mean colour of the lane's cell (channel 3 unused)
    __shared__ __attribute__((aligned(16))) float sO[16 * 4];
    __shared__ float sOut[64];
    __shared__ int sIdx[64];                                                    // the lane of the j-th packed cell
    const int lane = threadIdx.x;
    const int fr = lane & 15, kg = lane >> 4;
    const int K = a.K;
    const int opt = lane / 3, och = lane - opt * 3;                             // dense output role of a colour tile (ngp_rgb_chunks_kernel's)
    const float inv = 1.f / (float)SCENE_GRID_NDIR;
    f16x8_t ones = {(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
    if (kg == 0) { ones[0] = (_Float16)1.f; ones[1] = (_Float16)1.f; }
    for (long chunk = blockIdx.x; chunk < a.chunks; chunk += gridDim.x) {
        // ---- the lane's cell and its sample in the scene frame
        const long row = chunk / a.chunks_per_row;
        const int c0 = (int)(chunk - row * a.chunks_per_row) * 64 + lane;
        int ic[3];
        bool valid;
        if (a.lanes_z) {                                                        // row = ix ry + iy
            ic[0] = (int)(row / a.ry); ic[1] = (int)(row - (long)ic[0] * a.ry); ic[2] = c0;
            valid = c0 < a.rz;
        } else {                                                                // row = iy + ry iz
            ic[2] = (int)(row / a.ry); ic[1] = (int)(row - (long)ic[2] * a.ry); ic[0] = c0;
            valid = c0 < a.rx;
        }
        const long f = ((long)ic[0] * a.ry + ic[1]) * a.rz + ic[2];
        float xw[3] = {0.f, 0.f, 0.f};
        {
            const int rdim[3] = {a.rx, a.ry, a.rz};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float j = (a.jitter != nullptr && valid) ? a.jitter[f * 3 + k] : 0.5f;
                const float u = ((float)ic[k] + j) / (float)rdim[k];
                xw[k] = u * (a.hi[k] - a.lo[k]) + a.lo[k];
            }
        }
        // ---- coverage, weights, the blocks' densities (scene_field.h: scene_density_kernel's code), a_b = omega_b sigma_b
        unsigned mask;
        float del[FIELD_MAXB], om[FIELD_MAXB];
        scene_field_coverage(a.b, K, valid, xw, mask, del);
        scene_field_weights(mask, del, a.half_power, om);
        float sig[FIELD_MAXB] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int q = 0; q < K; ++q) {
            const bool have = (mask >> q) & 1u;
            if (!__any(have)) continue;
            const float s = scene_field_density<true>(a.b[q], have, xw, sH, sOut, &sF[q][0], lane);
#pragma unroll
            for (int j = 0; j < FIELD_MAXB; ++j) sig[j] = (j == q && have) ? s : sig[j];
            wave_sync();                                                        // sOut and the tile are rewritten by the next phase
        }
        float ab[FIELD_MAXB];
#pragma unroll
        for (int j = 0; j < FIELD_MAXB; ++j) ab[j] = om[j] * sig[j];
        const float sigma = ((ab[0] + ab[1]) + ab[2]) + ab[3];
        const float alpha = fminf(fmaxf(1.f - __expf(-a.delta * sigma), 0.f), 1.f);      // ngp_alpha_keep_kernel's arithmetic
        const bool kp = valid && sigma > a.thre;
        // ---- the colour of the kept cells: per block, the carriers packed into 16-point tiles
        float num[3] = {0.f, 0.f, 0.f}, den = 0.f, cbest[3] = {0.f, 0.f, 0.f}, abest = 0.f;
        int ncar = 0;
        bool bad = false;
        if (__any(kp)) {
#pragma unroll 1
            for (int q = 0; q < K; ++q) {
                float aq = 0.f;
#pragma unroll
                for (int j = 0; j < FIELD_MAXB; ++j) aq = (j == q) ? ab[j] : aq;
                const bool need = kp && aq != 0.f;
                const unsigned long long nm = __ballot(need);
                if (!nm) continue;
                const int cnt = __popcll(nm);
                if (need) sIdx[__popcll(nm & ((1ull << lane) - 1ull))] = lane;
                const SceneFieldBlock& b = a.b[q];
                const uint32_t* biaspk = a.biaspk[q];
                const _Float16* feat = &sF[q][0];
                NgpColorW cw;
                ngp_load_color_w(cw, b.cw1, b.cw2, b.cw3, lane);
                wave_sync();
#pragma unroll 1
                for (int t0 = 0; t0 < cnt; t0 += 16) {
                    {   // X = (0 x16 | feat[1..15] | 1) of the tile's point fr: lane (fr, kg) writes columns kg*4 .. +3 of both halves
                        typedef __attribute__((ext_vector_type(4))) _Float16 f16x4_t;
                        f16x4_t fv = {(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
                        if (t0 + fr < cnt) {
                            const int src = sIdx[t0 + fr];
#pragma unroll
                            for (int e = 0; e < 4; ++e) if (kg * 4 + e < 15) fv[e] = feat[src * 16 + 1 + kg * 4 + e];
                        }
                        if (kg == 3) fv[3] = (_Float16)1.f;
                        *reinterpret_cast<f16x4_t*>(sH + fr * NGP_XRS + kg * 8) = (f16x4_t){(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
                        *reinterpret_cast<f16x4_t*>(sH + fr * NGP_XRS + 32 + kg * 8) = fv;
                    }
                    const float sum = ngp_rgb_tile(cw, ones, biaspk, SCENE_GRID_NDIR, sH, sO, lane);
                    if (lane < 48 && t0 + opt < cnt) sC[sIdx[t0 + opt] * 4 + och] = sum * inv;
                    wave_sync();                                                // the tile is rewritten by the next one
                }
                if (need) {
                    const float c[3] = {sC[lane * 4], sC[lane * 4 + 1], sC[lane * 4 + 2]};
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const float pr = aq * c[ch];
                        bad = bad || !(fabsf(pr) <= 3.4028234664e38f);
                        num[ch] += pr;
                    }
                    den += aq;
                    ++ncar;
                    if (aq > abest) { abest = aq; cbest[0] = c[0]; cbest[1] = c[1]; cbest[2] = c[2]; }
                }
                wave_sync();                                                    // sIdx and sC are rewritten by the next block
            }
        }
        if (valid) {
            float row7[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (kp) {
                const bool own = ncar == 1 || bad || !(den <= 3.4028234664e38f);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    row7[k] = xw[k];
                    row7[3 + k] = ncar == 0 ? 0.f : (own ? cbest[k] : num[k] / den);
                }
                row7[6] = alpha;
            }
            float* g = a.grid + f * 7;
#pragma unroll
            for (int k = 0; k < 7; ++k) g[k] = row7[k];
            a.keep[f] = kp ? 1 : 0;
            if (a.sigma) a.sigma[f] = sigma;
        }
    }
}

static bool scene_grid_finite(float v) { return v - v == 0.f; }

extern "C" {

// The merged voxel grid of n_blocks registered blocks (HOST array `blocks`); see include/dreg_nerf.h.
int dreg_scene_voxel_grid(int rx, int ry, int rz, const float* grid_aabb, const float* jitter, int n_blocks, const dreg_radiance_block* blocks,
                          float power, float delta, float density_thre, float* voxel_grid, uint8_t* keep, float* sigma, void* stream)
{
    if (!grid_aabb || !blocks || !voxel_grid || !keep) return DREG_EINVAL;
    if (n_blocks < 1 || n_blocks > FIELD_MAXB) return DREG_EINVAL;
    if (rx < 1 || ry < 1 || rz < 1 || rx > 1024 || ry > 1024 || rz > 1024 || (long)rx * ry * rz > (1l << 28)) return DREG_EINVAL;
    for (int k = 0; k < 3; ++k) {
        const float ext = grid_aabb[3 + k] - grid_aabb[k];
        if (!scene_grid_finite(grid_aabb[k]) || !scene_grid_finite(grid_aabb[3 + k]) || !scene_grid_finite(ext) || !(ext > 0.f)) return DREG_EINVAL;
    }
    if (!scene_grid_finite(power) || !(power > 0.f) || !scene_grid_finite(delta) || !(delta > 0.f) || !scene_grid_finite(density_thre)) return DREG_EINVAL;
    SceneGridArgs a;
    __builtin_memset(&a, 0, sizeof(a));
    for (int b = 0; b < n_blocks; ++b) {
        const dreg_radiance_block& h = blocks[b];
        if (!h.cw1 || !h.cw2 || !h.cw3 || !h.dirbias) return DREG_EINVAL;
        if (scene_field_fill(a.b[b], h.field) != DREG_OK) return DREG_EINVAL;
        a.b[b].cw1 = (const _Float16*)h.cw1; a.b[b].cw2 = (const _Float16*)h.cw2; a.b[b].cw3 = (const _Float16*)h.cw3;
        a.biaspk[b] = reinterpret_cast<const uint32_t*>(h.dirbias) + SCENE_GRID_NDIR * 64;
    }
    a.K = n_blocks;
    a.half_power = 0.5f * power;
    a.rx = rx; a.ry = ry; a.rz = rz;
    a.lanes_z = g_scene_grid_lanes_z;
    a.chunks_per_row = ((a.lanes_z ? rz : rx) + 63) / 64;
    a.chunks = (long)a.chunks_per_row * ry * (a.lanes_z ? rx : rz);
    for (int k = 0; k < 3; ++k) { a.lo[k] = grid_aabb[k]; a.hi[k] = grid_aabb[3 + k]; }
    a.jitter = jitter;
    a.delta = delta; a.thre = density_thre;
    a.grid = voxel_grid; a.keep = keep; a.sigma = sigma;
    const long waves = a.chunks < g_scene_grid_waves ? a.chunks : g_scene_grid_waves;
    hipLaunchKernelGGL(scene_grid_kernel, dim3((unsigned)waves), dim3(64), 0, (hipStream_t)stream, a);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

#ifdef DREG_PROBE
void dreg_scene_grid_set_waves(int n) { g_scene_grid_waves = n > 0 ? n : 16384; }
void dreg_scene_grid_set_lanes_z(int on) { g_scene_grid_lanes_z = on ? 1 : 0; }
#endif

}  // extern "C"
