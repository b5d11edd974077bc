// What the kernels over a REGISTERED SCENE of K NeRF blocks share (gfx950, wave64): the density field (scene_field.hip) and the
// merged voxel grid (scene_grid.hip).  Stated here once:
//   * SceneFieldBlock, scene_field_fill — one block as these kernels read it (a MarchBlock, the centroid of its cameras, its pose rounded to
//                       fp32) and the ONE host function that validates and fills it from a dreg_field_block (through march_fill_block);
//   * scene_field_to_block, scene_field_covered — a scene-frame point in block b's frame, and b's own coverage of it;
//   * scene_field_coverage — all K coverages of the lane's point as a bit mask, and its squared distances to the blocks' camera centroids;
//   * scene_field_weights  — render_scene.hip's overlap weights from those (nothing is read per block);
//   * scene_field_density  — block b's density phase for the wave's 64 points: the 16-level gather of the covered lanes, the density MLP through
//                       one 64 x 64 fp16 LDS tile, sigma_b = __expf(h0 - 1) times the strictly-inside flag (the dense query's bits).  FEAT: the
//                       16 fp16 outputs of the net (h0 | 15 geometry features, the dense query's `raw` row) are left in sF as well.
// scene_density_kernel calls the coverage and the weights and keeps the density phase written out (through scene_field_density it took 119 instead
// of 117 VGPRs; it says so at the place); scene_grid_kernel calls all of them.  The rule itself is stated in the header of scene_field.hip.
// Every loop over the block index that reads a block stays ONE non-unrolled body that reads the block from the kernel-argument segment (render_pair.hip's header says why); nothing per lane is indexed by a run-time block index
// (that would go to scratch): per-block values sit in FIELD_MAXB named registers written by select inside unrolled loops.
#pragma once
#include "march.h"
#include "../../include/dreg_nerf.h"   // dreg_field_block, DREG_SCENE_MAX_BLOCKS

#define FIELD_MAXB DREG_SCENE_MAX_BLOCKS

struct SceneFieldBlock : MarchBlock {
    float center[3];            // centroid of the block's cameras, in the block's frame
    float R[9], t[3];           // the pose rounded to fp32: R row-major, then t (block -> scene); unused without a pose
    int has_pose;
};

// the scene-frame point x in block b's frame
__device__ __forceinline__ void scene_field_to_block(const SceneFieldBlock& b, const float (&x)[3], float (&xb)[3])
{
    if (b.has_pose) {
        const float d[3] = {x[0] - b.t[0], x[1] - b.t[1], x[2] - b.t[2]};
#pragma unroll
        for (int k = 0; k < 3; ++k) xb[k] = (b.R[k] * d[0] + b.R[3 + k] * d[1]) + b.R[6 + k] * d[2];
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) xb[k] = x[k];
    }
}

// whether block b's own occupancy grid covers the point x of its frame (the extents as march_grid forms them: the same fp32 subtraction)
__device__ __forceinline__ bool scene_field_covered(const MarchBlock& b, const float (&x)[3])
{
    const int rdim[3] = {b.rx, b.ry, b.rz};
    const float ext[3] = {b.roi[3] - b.roi[0], b.roi[4] - b.roi[1], b.roi[5] - b.roi[2]};
    return march_covered(b.roi, ext, rdim, b.binary, x);
}

// every block's own coverage of the lane's scene-frame point xw (a bit per block; none where !valid) and the point's squared distance to the
// block's camera centroid (1.f for the blocks >= K)
__device__ __forceinline__ void scene_field_coverage(const SceneFieldBlock* blocks, int K, bool valid, const float (&xw)[3], unsigned& mask,
                                                     float (&del)[FIELD_MAXB])
{
    mask = 0;
#pragma unroll
    for (int j = 0; j < FIELD_MAXB; ++j) del[j] = 1.f;
#pragma unroll 1
    for (int q = 0; q < K; ++q) {
        const SceneFieldBlock& b = blocks[q];
        float xb[3];
        scene_field_to_block(b, xw, xb);
        const bool m = valid && scene_field_covered(b, xb);
        float d = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) { const float e = xb[k] - b.center[k]; d += e * e; }
        d += 1e-12f;
        if (m) mask |= 1u << q;
#pragma unroll
        for (int j = 0; j < FIELD_MAXB; ++j) del[j] = (j == q) ? d : del[j];
    }
}

// the overlap weights (render_scene.hip's arithmetic; the distances are in registers: nothing is read per block)
__device__ __forceinline__ void scene_field_weights(unsigned mask, const float (&del)[FIELD_MAXB], float half_power, float (&om)[FIELD_MAXB])
{
#pragma unroll
    for (int j = 0; j < FIELD_MAXB; ++j) {
        float w = 0.f;
        if ((mask >> j) & 1u) {
            const unsigned others = mask & ~(1u << j);
            w = 1.f;
            if (others != 0) {
                if (__popc(others) == 1 && others < (1u << j)) {            // the one other block has the lower index: the pair's omega_hi = 1 - omega_lo
                    float d_lo = 1.f;
#pragma unroll
                    for (int i = 0; i < FIELD_MAXB; ++i) d_lo = ((others >> i) & 1u) ? del[i] : d_lo;
                    w = 1.f - 1.f / (1.f + __expf(half_power * __logf(d_lo / del[j])));
                } else {
                    float sum = 0.f;
#pragma unroll
                    for (int i = 0; i < FIELD_MAXB; ++i)
                        if (i != j && ((others >> i) & 1u)) sum += __expf(half_power * __logf(del[j] / del[i]));
                    w = 1.f / (1.f + sum);
                }
            }
        }
        om[j] = w;
    }
}

// Block b's density phase for the wave's 64 points: `have` = the lane's point is covered by b (the other lanes take a zero row), xw the lane's
// scene-frame point (x_b is recomputed from the same operands: the same bits).  sH: the wave's 64 x 64 fp16 tile (the encoded input lives in its
// first rows until the first layer has read it: ngp_density_kernel's layout), sOut: 64 floats.  Returns the dense query's density of the lane's
// point (whatever `have`: the caller selects).  FEAT: row `lane` of sF (64 rows of 16 fp16, apart from sH) receives the net's 16 outputs rounded
// to fp16 — the `raw` row of the dense query (h0 | 15 geometry features).  The caller's wave_sync() follows before sOut / the tile are rewritten.
template <bool FEAT>
__device__ __forceinline__ float scene_field_density(const SceneFieldBlock& b, bool have, const float (&xw)[3], char* sH, float* sOut, _Float16* sF, int lane)
{
    char* sX = sH;
    const int fr = lane & 15, kg = lane >> 4;
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
        if constexpr (FEAT) {
#pragma unroll
            for (int r = 0; r < 4; ++r) sF[(rb * 16 + kg * 4 + r) * 16 + fr] = (_Float16)ov[r];
        }
    });
    wave_sync();
    return __expf(sOut[lane] - 1.f) * (inside_m ? 1.f : 0.f);          // the dense query's density (ngp_density_kernel)
}

static inline int scene_field_fill(SceneFieldBlock& b, const dreg_field_block& h)
{
    if (!h.center) return DREG_EINVAL;
    for (int k = 0; k < 3; ++k) b.center[k] = h.center[k];
    b.has_pose = h.pose != nullptr;
    for (int k = 0; k < 9; ++k) b.R[k] = h.pose ? h.pose[k] : 0.f;
    for (int k = 0; k < 3; ++k) b.t[k] = h.pose ? h.pose[9 + k] : 0.f;
    // no ray is marched: no colour net, no scene interval (the roi stands in for the scene aabb, the step for a positive number)
    return march_fill_block(b, h.binary, h.rx, h.ry, h.rz, nullptr, h.table, h.w1, h.w2, false, nullptr, nullptr, nullptr, h.offset, h.size, h.res, h.scale,
                            h.hashed, h.roi_aabb, h.roi_aabb, h.model_aabb, 0.f, 0.f, 1.f, 0.f, false);
}
