// The backward of a NeRF block's field (hash-grid encoding, density net, colour net), stated once for the kernels that train it or differentiate
// it (gfx950, wave64): the render backward (render_train.hip), the point backward (field_train.hip) and the input gradients
// (field_input_grad.hip).  The forward these kernels recompute is ngp_field.h's and march.h's.  Stated here:
//   * the parameter layout — the five matrices in parameter order and the table's start: the split of mlp_base.params / color_mlp.params
//                       (ngp_split_params) and the offsets of a weight-gradient slab are written from the same constants;
//   * fb_layout       — the chunk rule (64 items per chunk up to 131,072 items, at most 2,048 chunks: it depends on n only) and the workspace
//                       (an optional lead, one slab per chunk, the chunk queue);  fb_next_chunk — a wave's next chunk from the queue;
//   * fb_outer        — the weight gradient of one layer: the sum over the wave's 64 items of dY x X on v_mfma_f32_16x16x4_f32, added into the
//                       chunk's own slab (the wave owns it: plain loads and stores);
//   * fb_reduce       — the slabs summed in chunk order into the two parameter gradients: bit-identical between runs and launch widths;
//   * fb_back, fb_store — dX = dY W on the same MFMA through the fp32 LDS tile sA [64 items][<= 64 units], and its store back into sA gated by
//                       the ReLU of the layer below (FbGateLds: the fp16 hidden rows still in LDS; FbGateMask: a lane mask fetched by shuffle);
//   * FieldPointArgs, field_fill_points, field_point_forward — a launch over POINTS with two upstream gradients: the shared head of the
//                       kernel arguments, the ONE host function that validates and fills it, and the recomputed forward of a wave's 64 points
//                       up to dL/d(colour pre-activation) and dL/dh0.
// Deliberately left apart: ngp_render_bwd_kernel keeps its per-lane VALU chain (d2, d1, dout, dh, de in registers) and takes only the layout,
// the chunking, fb_outer and fb_reduce from here; on the MFMA chain its sums would be formed in another order.
#pragma once
#include "march.h"

// ---- parameter layout: mlp_base.params = density W1 [64][32] | W2 [16][64] | hash table;  color_mlp.params = colour W1 [64][32] | W2 [64][64] | W3 [16][64]
constexpr int NGP_BASE_W1 = 0, NGP_BASE_W2 = NGP_BASE_W1 + 64 * 32, NGP_BASE_TABLE = NGP_BASE_W2 + 16 * 64;
constexpr int NGP_COLOR_W1 = 0, NGP_COLOR_W2 = NGP_COLOR_W1 + 64 * 32, NGP_COLOR_W3 = NGP_COLOR_W2 + 64 * 64, NGP_COLOR_END = NGP_COLOR_W3 + 16 * 64;
// one slab = the five weight matrices in parameter order (the density net's, then the colour net's), fp32
constexpr int FB_OFF_D1 = NGP_BASE_W1, FB_OFF_D2 = NGP_BASE_W2, FB_OFF_C1 = NGP_BASE_TABLE, FB_OFF_C2 = FB_OFF_C1 + NGP_COLOR_W2,
              FB_OFF_C3 = FB_OFF_C1 + NGP_COLOR_W3, FB_SLAB = FB_OFF_C1 + NGP_COLOR_END;
constexpr long FB_MAX_CHUNKS = 2048;
constexpr int FB_AS = 68;              // row stride (floats) of the wave's fp32 tile sA [64 items][<= 64 units]
static_assert(FB_SLAB % 256 == 0, "fb_reduce launches FB_SLAB / 256 workgroups of 256");

struct NgpParams16 { const _Float16 *table, *w1, *w2, *cw1, *cw2, *cw3; };
static inline NgpParams16 ngp_split_params(const void* base16, const void* color16)
{
    const _Float16* b = (const _Float16*)base16;
    const _Float16* c = (const _Float16*)color16;
    return {b + NGP_BASE_TABLE, b + NGP_BASE_W1, b + NGP_BASE_W2, c + NGP_COLOR_W1, c + NGP_COLOR_W2, c + NGP_COLOR_W3};
}

// ---- chunks and workspace: [lead bytes (the caller's own)] [n_chunks slabs] [queue: 256 bytes]; slabs and queue are zeroed by the entry point
struct FbLayout { long chunk_items; int n_chunks; size_t slab_off, queue_off, total; };
static inline int fb_layout(long n, size_t lead, FbLayout& w)
{
    if (n <= 0) return DREG_EINVAL;
    const long waves = (n + 63) / 64;
    w.chunk_items = 64 * ((waves + FB_MAX_CHUNKS - 1) / FB_MAX_CHUNKS);
    w.n_chunks = (int)((n + w.chunk_items - 1) / w.chunk_items);
    w.slab_off = lead;
    w.queue_off = lead + (size_t)w.n_chunks * FB_SLAB * sizeof(float);
    w.total = w.queue_off + 256;
    return DREG_OK;
}

// the wave's next chunk (one atomic per chunk); >= n_chunks: the queue is empty
__device__ __forceinline__ unsigned int fb_next_chunk(unsigned int* queue, int lane)
{
    unsigned int chunk = 0;
    if (lane == 0) chunk = atomicAdd(queue, 1u);
    return __shfl(chunk, 0, 64);
}

// ---- weight gradient of one layer
// W[m][n] += sum_s sA[s][m] X(s, n) over the wave's 64 items, for the MT x NT 16x16 tiles of W (row stride ld) in the chunk's slab.  X: fp16 LDS
// rows of stride xrs.  LIVE: X is masked by sLive (rows of items that are not live are not read: they may hold anything).  UNROLL: the tile
// loops are unrolled in full (the render backward, at its register limit, compiles to less scratch this way) or kept as loops.
template <int MT, int NT, bool LIVE, bool UNROLL>
__device__ __forceinline__ void fb_outer(float* slab, int ld, const float* sA, const char* sXin, int xrs, const float* sLive, int lane)
{
    const int fr = lane & 15, kq = lane >> 4;
    auto tile = [&](int mt, int nt) {
        f32x4_t acc = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int kk = 0; kk < 16; ++kk) {
            const int s = kk * 4 + kq;
            const float xv = !LIVE || sLive[s] != 0.f ? (float)reinterpret_cast<const _Float16*>(sXin + s * xrs)[nt * 16 + fr] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(sA[s * FB_AS + mt * 16 + fr], xv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) slab[(mt * 16 + kq * 4 + r) * ld + nt * 16 + fr] += acc[r];    // W[mt*16 + kq*4 + r][nt*16 + fr]
    };
    if constexpr (UNROLL) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) tile(mt, nt);
    } else {
#pragma unroll 1
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll 1
            for (int nt = 0; nt < NT; ++nt) tile(mt, nt);
    }
}

// grad[e] += sum over chunks (in chunk order) of slab[c][e]: base = mlp_base.params[0 : NGP_BASE_TABLE] gradient, color = color_mlp.params gradient.
// One launch on `stream`; DREG_OK or the launch error.  The kernel and this launcher are defined in field_train.hip.
int fb_reduce(const float* slabs, int n_chunks, float* grad_base, float* grad_color, hipStream_t stream);

// ---- dX = dY W
// dX[p][c0 + i] = sum_{k < 4 KS} sA[p][k] W[k][c0 + i], i < 16 NT, for the wave's 64 items (W: fp16 [.][ld], rows = the layer's outputs).
// acc[pt][nt][r] = dX of item pt*16 + (lane >> 4)*4 + r, column c0 + nt*16 + (lane & 15).
template <int KS, int NT>
__device__ __forceinline__ void fb_back(f32x4_t (&acc)[4][NT], const float* sA, const _Float16* __restrict__ W, int ld, int c0, int lane)
{
    const int fr = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[pt][nt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int ks = 0; ks < KS; ++ks) {
        float b[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) b[nt] = (float)W[(ks * 4 + kq) * ld + c0 + nt * 16 + fr];
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) {
            const float av = sA[(pt * 16 + fr) * FB_AS + ks * 4 + kq];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[pt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[nt], acc[pt][nt], 0, 0, 0);
        }
    }
}

// Where fb_store takes relu'(h) of item p, unit c from: row(p) once per item (every lane calls it), on(row, c) per unit.
struct FbGateNone {                    // no gate
    __device__ __forceinline__ int row(int) const { return 0; }
    __device__ __forceinline__ bool on(int, int) const { return true; }
};
struct FbGateLds {                     // the fp16 hidden rows of the forward, still in LDS (stride NGP_HRS)
    const char* sH;
    __device__ __forceinline__ const _Float16* row(int p) const { return reinterpret_cast<const _Float16*>(sH + p * NGP_HRS); }
    __device__ __forceinline__ bool on(const _Float16* h, int c) const { return (float)h[c] > 0.f; }
};
struct FbGateMask {                    // ngp_relu_mask of the lane's own item, held by that lane: another item's is fetched with a shuffle
    unsigned long long mask;
    __device__ __forceinline__ unsigned long long row(int p) const { return __shfl(mask, p, 64); }
    __device__ __forceinline__ bool on(unsigned long long m, int c) const { return (m >> c) & 1ull; }
};
// acc -> sA columns 0 .. 16 NT - 1, gated
template <int NT, class Gate>
__device__ __forceinline__ void fb_store(float* sA, const f32x4_t (&acc)[4][NT], const Gate& gate, int lane)
{
    const int fr = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = pt * 16 + kq * 4 + r;
            const auto g = gate.row(p);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int c = nt * 16 + fr;
                sA[p * FB_AS + c] = gate.on(g, c) ? acc[pt][nt][r] : 0.f;
            }
        }
}

// ---- a launch over points: x, unit directions, and the upstream gradients dL/dsigma [n] and dL/drgb [n,3]
struct FieldPointArgs {                // the head of the kernel arguments; field_fill_points writes every field
    const float *x, *dirs;
    long n;
    const _Float16 *table, *w1, *w2, *cw1, *cw2, *cw3;
    NgpLevels lv;
    float model[6];
    const float *g_sigma, *g_rgb;      // either may be null (zeros)
};
// Validate and fill the head from an entry point's own arguments (n > 0): DREG_OK, or DREG_EINVAL with nothing launched.
static inline int field_fill_points(FieldPointArgs& a, const float* x, const float* dirs, long n, const void* base16, const void* color16,
                                    const uint32_t* offset, const uint32_t* size, const uint32_t* res, const float* scale, const uint32_t* hashed,
                                    const float* model_aabb, const float* g_sigma, const float* g_rgb)
{
    if (!x || !dirs || !base16 || !color16 || !offset || !size || !res || !scale || !hashed || !model_aabb) return DREG_EINVAL;
    for (int k = 0; k < 3; ++k)
        if (!(model_aabb[3 + k] > model_aabb[k])) return DREG_EINVAL;
    const NgpParams16 w = ngp_split_params(base16, color16);
    a.x = x; a.dirs = dirs; a.n = n;
    a.table = w.table; a.w1 = w.w1; a.w2 = w.w2; a.cw1 = w.cw1; a.cw2 = w.cw2; a.cw3 = w.cw3;
    ngp_fill_levels(a.lv, offset, size, res, scale, hashed);
    for (int k = 0; k < 6; ++k) a.model[k] = model_aabb[k];
    a.g_sigma = g_sigma; a.g_rgb = g_rgb;
    return DREG_OK;
}

// One lane's point of a wave's 64, and what the forward leaves of it for the chain.
struct FieldPoint {
    float x[3], d[3], gs, gc[3];       // the point and its upstream gradients (zeros where have is false)
    bool live;                         // some upstream gradient of the point is not zero
    float u[3];                        // unit-cube coordinates in the model aabb, clamped
    bool inside_m;                     // strictly inside the model aabb
    float dO[3], dh0;                  // dL/d(colour pre-activation), dL/dh0
};
// Load point p (have: the lane has one) and recompute the forward of the wave's 64 points exactly as inference does (ngp_field.h, march.h):
// hash gather -> sE, density net sE -> sHd with h0 -> sOut and the 15 features -> columns 16..30 of sX, fp16 SH4(d) | . | 1 -> sX, colour net
// sX -> sH1 -> sH2 -> sO; then dL/do_c = g_rgb_c c (1 - c) and dL/dh0 = g_sigma exp(min(h0 - 1, 15)) inside the model aabb.  Lanes without a
// point take zero rows: every LDS row is written and finite.  False (wave-uniform): no gradient arrives at these 64 points and nothing was
// computed.  The tiles are the caller's and may alias as ngp_density_mlp and march_color allow (sE inside sHd; sH1 = sHd; sX inside sH2);
// after_density() runs between the two nets, when sHd holds the density net's hidden rows and before anything overwrites them.
template <class Hook>
__device__ __forceinline__ bool field_point_forward(const FieldPointArgs& a, long p, bool have, char* sE, char* sHd, char* sX, char* sH1, char* sH2,
                                                    float* sOut, float* sO, int lane, FieldPoint& pt, Hook&& after_density)
{
    const int fr = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int k = 0; k < 3; ++k) { pt.x[k] = 0.f; pt.d[k] = 0.f; pt.gc[k] = 0.f; }
    pt.gs = 0.f;
    if (have) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { pt.x[k] = a.x[p * 3 + k]; pt.d[k] = a.dirs[p * 3 + k]; }
        if (a.g_sigma) pt.gs = a.g_sigma[p];
        if (a.g_rgb) {
#pragma unroll
            for (int k = 0; k < 3; ++k) pt.gc[k] = a.g_rgb[p * 3 + k];
        }
    }
    pt.live = pt.gs != 0.f || pt.gc[0] != 0.f || pt.gc[1] != 0.f || pt.gc[2] != 0.f;
    if (!__any(pt.live)) return false;
    pt.inside_m = ngp_unit_cube(pt.x, a.model, a.model + 3, 0, pt.u) && have;
    {
        _Float16* er = reinterpret_cast<_Float16*>(sE + lane * NGP_XRS);
#pragma unroll 2
        for (int l = 0; l < 16; ++l) {
            float f0 = 0.f, f1 = 0.f;
            if (have) ngp_level_features(a.table, a.lv, l, pt.u, f0, f1);
            er[2 * l] = (_Float16)f0; er[2 * l + 1] = (_Float16)f1;
        }
        NgpDensityW dw;
        ngp_load_density_w(dw, a.w1, a.w2, lane);
        ngp_density_mlp(dw, sE, sHd, lane, [&](int rb, const f32x4_t& ov) {      // ov[r] = output fr of point rb*16 + kq*4 + r
            if (fr == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) sOut[rb * 16 + kq * 4 + r] = (float)(_Float16)ov[r];
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) reinterpret_cast<_Float16*>(sX + (rb * 16 + kq * 4 + r) * NGP_XRS)[15 + fr] = (_Float16)ov[r];
            }
        });
        after_density();
        uint32_t sh2[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) sh2[j] = 0u;
        if (have) render_sh4_f16(pt.d, sh2);
        march_color_row(sX, lane, sh2);
        f16x8_t cw1f[4], cw3f[2];
        march_load_color_w(cw1f, cw3f, a.cw1, a.cw3, lane);
        march_color(sX, sH1, sH2, sO, cw1f, a.cw2, cw3f, lane);
    }
    pt.dh0 = 0.f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float c = march_sigmoid_f16(sO[lane * 4 + ch]);
        pt.dO[ch] = pt.gc[ch] * c * (1.f - c);
    }
    if (pt.inside_m) pt.dh0 = pt.gs * __expf(fminf(sOut[lane] - 1.f, 15.f));
    return true;
}
