// Row-panel kernels of the point-set half's encoder layers (gfx950): between two attention calls every operation is row-local, so ONE
// workgroup that owns a panel of 64 rows runs a whole chain with no synchronisation outside the workgroup:
//   forward   x = A1 W1^T + bias1 + residual (fp32)  ->  h = LayerNorm(x) (+pe) (bf16)       ->  out2 = h W2^T + bias2 (ReLU) (bf16)
//   backward  dH = G1 W1 (bf16)                      ->  dx = LayerNorm'(dH) + by-passing gradients (fp32, bf16 copy, dgamma / dbeta
//                                                        partials per 16 rows)                ->  out2 = dx_bf16 W2 (bf16; optional)
// One launch fill / drain instead of three, and the intermediate is never read back from memory (x, h and dx are still WRITTEN to the
// arena: later launches read them; dH was scratch of the chain and is not written at all).
//
// Bit-identity with the launches a chain replaces (conv_igemm_glds_kernel 1x1x1 -> layernorm_{fwd,bwd}_kernel -> conv_igemm_glds_kernel)
// is the design constraint: the linear layers never take split-K, so every output element there is one in-order chain of
// mfma_f32_16x16x32_bf16 over K.  These kernels keep the operand roles (weights as the MFMA's first operand), the k-slot layout (lane
// group kg of fragment ks holds channels 64 k + 32 ks + 8 kg .. + 7 of stage k), the stage order, the rounding points (x and dx fp32;
// h, dH, the bf16 copy of dx and out2 bf16), the epilogue's order of additions (+bias, then +residual), the LayerNorm row arithmetic
// (ln_rows_fwd / ln_rows_bwd of common.h, shared with pointset.hip) and the order of the dgamma / dbeta sums (rows w, w + 4, w + 8,
// w + 12 of a 16-row block per partial, the four partials added left to right).  Which rows share a workgroup changes nothing:
// tests/test_hip_pointset_panel.py.
#include "common.h"
#include "../../include/dreg_nerf.h"

namespace {

constexpr int PM = 64;                       // rows per panel
constexpr int PC = 256;                      // LayerNorm width = GEMM1's outputs = GEMM2's K = GEMM2's outputs per chunk
constexpr int PNW = 8;                       // waves: wave w forms channels 32 w .. 32 w + 31 of all 64 rows (4 x 2 MFMA tiles)
constexpr int W_BYTES = PC * 128, A_BYTES = PM * 128, STG = W_BYTES + A_BYTES;   // one 64-channel stage: weights [256][64], activations [64][64]
// LDS.  GEMM1 streams (weights, activations) through a ring of three stages in [0, 120 K).  Afterwards: the fp32 tile [64][256] of its
// results in [0, 64 K); h (the bf16 result of the row pass, GEMM2's activation operand) in [64 K, 96 K); GEMM2 streams weight stages
// through the ring P0 = [96 K, 128 K) -> [0, 32 K) -> [32 K, 64 K) -> [64 K, 96 K) (h lives in registers by then: three stages are in
// flight while one is consumed).  P0 is free during the row pass, so stage 0 is already on its way then (forward; the backward row
// pass keeps its dgamma / dbeta partials there).  GEMM2's bias sits behind all of it: every memory
// operation of GEMM2's loop is then a weight-stage load or an output store, which its counted waits rely on.
constexpr int H_OFF = 64 * 1024, P0_OFF = 96 * 1024, B2_OFF = 128 * 1024, MAX_N2 = 1024, PANEL_LDS = B2_OFF + MAX_N2 * 4;   // + GEMM2's bias (forward)
static_assert(3 * STG <= B2_OFF && PM * PC * 4 <= H_OFF && H_OFF + PM * PC * 2 <= P0_OFF && P0_OFF + W_BYTES <= B2_OFF && PANEL_LDS <= 160 * 1024, "LDS plan");

struct PanelArgs {
    const bf16_t* a1; const bf16_t* w1; const bf16_t* w2; bf16_t* out2;      // GEMM1's activations [R][K1] and pack [256][K1]; GEMM2's pack [N2][256], output [R][N2]
    int R, K1, N2, relu;
    float eps;
    const float* gamma;
    // forward row pass
    const float* bias1; const float* residual; float* xout; const float* beta; const float* pe; bf16_t* hout; float* stats; const float* bias2;
    // backward row pass (dx may alias dx_add / dx_add2: a row is read and written by the same wave)
    const float* x; const float* st; const float* dx_add; const float* dx_add2; float* dx; bf16_t* dx_bf; float* part;
};

// Workgroup barrier that does NOT drain the vector-memory counter: __syncthreads() waits for every outstanding load of the wave, i.e. for
// the stages requested ahead, and the ring would run one load latency per stage.  LDS traffic of this wave is complete before it
// arrives; what must have landed from memory is waited for explicitly (counted s_waitcnt vmcnt) in front of each barrier.  The waves of
// a panel hand nothing to each other through global memory.
__device__ __forceinline__ void wg_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

__device__ __forceinline__ uint32_t pswz(int row, int slot) { return (uint32_t)row * 128u + (uint32_t)((slot ^ ((row >> 1) & 7)) << 4); }

template <bool BWD>
__global__ __launch_bounds__(PNW * 64) void ps_panel_kernel(const PanelArgs a)
{
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    constexpr uint32_t OOB = 0x7fffff00u;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int m0 = blockIdx.x * PM;
    const int fr = lane & 15, kg = lane >> 4;
    const int R = a.R, K1 = a.K1, N2 = a.N2;

    const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc((void*)a.a1, 0, (uint32_t)R * (uint32_t)(K1 * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_w1 = __builtin_amdgcn_make_buffer_rsrc((void*)a.w1, 0, (uint32_t)(PC * K1 * 2), 0x00020000);
    // (stores of rows beyond R are out of range of this descriptor: the hardware drops them, and every wave issues the same number of stores)
    const __amdgpu_buffer_rsrc_t rs_o2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.out2, 0, (uint32_t)R * (uint32_t)(N2 * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_w2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.w2, 0, (uint32_t)(N2 * PC * 2), 0x00020000);

    // staging roles (direct-to-LDS, 16 bytes per lane, 8 rows x 8 granules per wave-instruction; the XOR swizzle is applied on the source
    // side, as in conv_igemm_glds_kernel): this wave brings weight rows (wave * 4 + i) * 8 + (lane >> 3) and activation row wave * 8 + (lane >> 3)
    uint32_t wrow[4], wgl[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (wave * 4 + i) * 8 + (lane >> 3);
        wrow[i] = (uint32_t)r;
        wgl[i] = (uint32_t)(((lane & 7) ^ ((r >> 1) & 7)) * 16);
    }
    uint32_t avoff;
    {
        const int r = wave * 8 + (lane >> 3);
        const int gl = (lane & 7) ^ ((r >> 1) & 7);
        avoff = (m0 + r < R) ? (uint32_t)(m0 + r) * (uint32_t)(K1 * 2) + (uint32_t)(gl * 16) : OOB;   // rows beyond R: the raw buffer's bounds check returns zeros
    }

    // ---- the row pass's operands from memory are requested first: they arrive while GEMM1 runs.  A wave's 8 rows:
    // forward 8 w + q; backward the rows of TWO of layernorm_bwd_kernel's waves (block w >> 1 of 16 rows, its waves 2 (w & 1) + vv: rows vw + 4 u)
    constexpr int RPW = PM / PNW;
    auto row_of = [&](int q) -> int { return BWD ? (wave >> 1) * 16 + (wave & 1) * 2 + (q >> 2) + 4 * (q & 3) : wave * RPW + q; };
    float4 r0[RPW], r1[RPW], r2[RPW];          // forward: residual, pe;  backward: x, dx_add, dx_add2
    float mean_[RPW], rstd_[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        const int row = m0 + row_of(q);
        r0[q] = make_float4(0.f, 0.f, 0.f, 0.f); r1[q] = r0[q]; r2[q] = r0[q]; mean_[q] = 0.f; rstd_[q] = 0.f;
        if (row < R) {
            const size_t o = (size_t)row * PC + lane * 4;
            if constexpr (BWD) {
                r0[q] = *reinterpret_cast<const float4*>(a.x + o);
                if (a.dx_add) r1[q] = *reinterpret_cast<const float4*>(a.dx_add + o);
                if (a.dx_add2) r2[q] = *reinterpret_cast<const float4*>(a.dx_add2 + o);
                mean_[q] = a.st[2 * row]; rstd_[q] = a.st[2 * row + 1];
            } else {
                r0[q] = *reinterpret_cast<const float4*>(a.residual + o);
                if (a.pe) r1[q] = *reinterpret_cast<const float4*>(a.pe + o);
            }
        }
    }

    const float4 gg = *reinterpret_cast<const float4*>(a.gamma + lane * 4);
    float4 b1 = make_float4(0.f, 0.f, 0.f, 0.f), bb = b1, b2v = b1;
    if constexpr (!BWD) {
        b1 = *reinterpret_cast<const float4*>(a.bias1 + lane * 4); bb = *reinterpret_cast<const float4*>(a.beta + lane * 4);
        if (t * 4 < N2) b2v = *reinterpret_cast<const float4*>(a.bias2 + t * 4);     // (into LDS once GEMM1's loads have been requested)
    }

    f32x4_t acc[4][2];
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    };

    // ---------------------------------------------------------------- GEMM1: A1 W1^T, K1 / 64 stages of (W1 [256][64], A1 [64][64])
    {
        const int nk = K1 >> 6;
        auto issue = [&](int k, int buf) {
            char* sW = smem + buf * STG + wave * 4096;
            char* sA = smem + buf * STG + W_BYTES + wave * 1024;
            const uint32_t so = (uint32_t)(k * 128);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w1, (lds_ptr_t)(sW + i * 1024), 16, (int)(wrow[i] * (uint32_t)(K1 * 2) + wgl[i]), (int)so, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a, (lds_ptr_t)sA, 16, (int)avoff, (int)so, 0, 0);
        };
        zero_acc();
        for (int s = 0; s < 2 && s < nk; ++s) issue(s, s);
        int cbuf = 0, ibuf = 2;
        for (int k = 0; k < nk; ++k) {
            // this wave's pieces of stage k have landed: loads retire in order, so at most the five of stage k + 1 are still in flight
            // (the row-pass operands were requested before stage 0)
            if (k + 1 < nk) asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            wg_barrier();                               // stage k landed for every wave; everyone is done with stage k - 1
            if (k + 2 < nk) issue(k + 2, ibuf);
            const char* sW = smem + cbuf * STG;
            const char* sA = sW + W_BYTES;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8_t af[4], bf[2];
#pragma unroll
                for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const bf16x8_t*>(sA + pswz(i * 16 + fr, ks * 4 + kg));
#pragma unroll
                for (int j = 0; j < 2; ++j) bf[j] = *reinterpret_cast<const bf16x8_t*>(sW + pswz(wave * 32 + j * 16 + fr, ks * 4 + kg));
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[j], af[i], acc[i][j], 0, 0, 0);   // C^T: a lane holds 4 consecutive channels of one row
            }
            cbuf = cbuf == 2 ? 0 : cbuf + 1;
            ibuf = ibuf == 2 ? 0 : ibuf + 1;
        }
    }
    // accumulators -> fp32 tile [64][256] (16-byte granules XOR-ed with the row's low four bits: the 16 lanes of a write phase, 16 rows
    // of the same channels, land in 16 different granules)
    float* sC = reinterpret_cast<float*>(smem);
    wg_barrier();                                          // every wave is done with the ring
    if constexpr (!BWD) { if (t * 4 < N2) *reinterpret_cast<float4*>(smem + B2_OFF + t * 16) = b2v; }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = i * 16 + fr;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int gr = ((wave * 32 + j * 16) >> 2) + kg;
            *reinterpret_cast<f32x4_t*>(sC + row * PC + ((gr ^ fr) << 2)) = acc[i][j];
        }
    }
    // GEMM2's weight stages: ring slot of stage s
    const int nst = (N2 >> 8) * 4;
    auto slot2 = [&](int s) -> char* { const int m = s & 3; return smem + (m == 0 ? P0_OFF : m == 3 ? H_OFF : (m - 1) * W_BYTES); };
    auto issue2 = [&](int s) {
        char* sW = slot2(s) + wave * 4096;
        const uint32_t so = (uint32_t)((s >> 2) * (PC * PC * 2) + (s & 3) * 128);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w2, (lds_ptr_t)(sW + i * 1024), 16, (int)(wrow[i] * (uint32_t)(PC * 2) + wgl[i]), (int)so, 0, 0);
    };
    if constexpr (!BWD) { if (nst > 0) issue2(0); }
    wg_barrier();

    // ---------------------------------------------------------------- the row pass: one wave per row, lane l = channels 4l .. 4l + 3
    // the row's bf16 result into h: channels 4l .. 4l + 3 = k-chunk l >> 4, 16-byte granule (l & 15) >> 1 of the row's 128 bytes, its low or high half
    auto put_h = [&](int lrow, uint2 hb) { *reinterpret_cast<uint2*>(smem + H_OFF + (lane >> 4) * A_BYTES + pswz(lrow, (lane & 15) >> 1) + (lane & 1) * 8) = hb; };
    // The wave's 8 rows go through the reductions TOGETHER (ln_rows_*: the shuffles of a step back to back): one row after the other was a
    // chain of 12 dependent cross-lane steps per row, 6 us of a 25 us launch.  Rows beyond R are computed on zeros and not stored.
    float4 cv[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) { const int lrow = row_of(q); cv[q] = *reinterpret_cast<const float4*>(sC + lrow * PC + ((lane ^ (lrow & 15)) << 2)); }
    if constexpr (!BWD) {
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            cv[q].x += b1.x; cv[q].y += b1.y; cv[q].z += b1.z; cv[q].w += b1.w;
            cv[q].x += r0[q].x; cv[q].y += r0[q].y; cv[q].z += r0[q].z; cv[q].w += r0[q].w;
        }
        float o[RPW][4], mean[RPW], rstd[RPW];
        ln_rows_fwd<RPW>(cv, gg, bb, a.eps, o, mean, rstd);
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            const int lrow = row_of(q), row = m0 + lrow;
            if (a.pe) { o[q][0] += r1[q].x; o[q][1] += r1[q].y; o[q][2] += r1[q].z; o[q][3] += r1[q].w; }
            const uint2 hb = make_uint2(f2bf2(o[q][0], o[q][1]), f2bf2(o[q][2], o[q][3]));
            put_h(lrow, hb);
            if (row < R) {                                 // (wave-uniform)
                *reinterpret_cast<float4*>(a.xout + (size_t)row * PC + lane * 4) = cv[q];
                *reinterpret_cast<uint2*>(a.hout + (size_t)row * PC + lane * 4) = hb;
                if (lane == 0) { a.stats[2 * row] = mean[q]; a.stats[2 * row + 1] = rstd[q]; }
            }
        }
    } else {
        const float gv[4] = {gg.x, gg.y, gg.z, gg.w};
        float* red = reinterpret_cast<float*>(smem + P0_OFF);          // [4 blocks of 16 rows][4 waves of layernorm_bwd_kernel][512]
        float d[RPW][4], xh[RPW][4], o[RPW][4];
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            const uint32_t w0 = f2bf2(cv[q].x, cv[q].y), w1 = f2bf2(cv[q].z, cv[q].w);      // dH is a bf16 tensor in the chain this replaces
            d[q][0] = __uint_as_float(w0 << 16); d[q][1] = __uint_as_float(w0 & 0xffff0000u); d[q][2] = __uint_as_float(w1 << 16); d[q][3] = __uint_as_float(w1 & 0xffff0000u);
        }
        ln_rows_bwd<RPW>(r0, d, mean_, rstd_, gv, xh, o);
#pragma unroll
        for (int vv = 0; vv < 2; ++vv) {
            float dg[4] = {0.f, 0.f, 0.f, 0.f}, db[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = vv * 4 + u;
                const int lrow = row_of(q), row = m0 + lrow;
                const bool valid = row < R;                // (wave-uniform) rows beyond R add nothing, as in layernorm_bwd_kernel
#pragma unroll
                for (int i = 0; i < 4; ++i) { dg[i] = valid ? dg[i] + d[q][i] * xh[q][i] : dg[i]; db[i] = valid ? db[i] + d[q][i] : db[i]; }
                if (a.dx_add) { o[q][0] += r1[q].x; o[q][1] += r1[q].y; o[q][2] += r1[q].z; o[q][3] += r1[q].w; }
                if (a.dx_add2) { o[q][0] += r2[q].x; o[q][1] += r2[q].y; o[q][2] += r2[q].z; o[q][3] += r2[q].w; }
                const uint2 hb = make_uint2(f2bf2(o[q][0], o[q][1]), f2bf2(o[q][2], o[q][3]));
                put_h(lrow, hb);
                if (valid) {
                    *reinterpret_cast<float4*>(a.dx + (size_t)row * PC + lane * 4) = make_float4(o[q][0], o[q][1], o[q][2], o[q][3]);
                    if (a.dx_bf) *reinterpret_cast<uint2*>(a.dx_bf + (size_t)row * PC + lane * 4) = hb;
                }
            }
            float* rw = red + ((wave >> 1) * 4 + (wave & 1) * 2 + vv) * 512;
#pragma unroll
            for (int i = 0; i < 4; ++i) { rw[lane * 4 + i] = dg[i]; rw[256 + lane * 4 + i] = db[i]; }
        }
        wg_barrier();
        // partials of the 16-row blocks that hold a row (the workspace ends with the last of them)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (m0 + b * 16 >= R) break;
            const float* rb = red + b * 4 * 512 + t;
            a.part[(size_t)((m0 >> 4) + b) * 512 + t] = rb[0] + rb[512] + rb[1024] + rb[1536];
        }
    }
    wg_barrier();                                       // h complete; the fp32 tile (and the partials) are dead
    if (nst == 0) return;

    // ---------------------------------------------------------------- GEMM2: out2 = h W2^T in chunks of 256 outputs, 4 stages of W2 [256][64] each
    if constexpr (BWD) issue2(0);
    issue2(1);
    issue2(2);                                             // (nst is a multiple of 4)
    bf16x8_t ah[8][4];                                     // this wave's fragments of h (all 64 rows, K = 256): read once, used by every chunk
#pragma unroll
    for (int kk = 0; kk < 8; ++kk)
#pragma unroll
        for (int i = 0; i < 4; ++i) ah[kk][i] = *reinterpret_cast<const bf16x8_t*>(smem + H_OFF + (kk >> 1) * A_BYTES + pswz(i * 16 + fr, (kk & 1) * 4 + kg));
    zero_acc();
    for (int c = 0; c < (N2 >> 8); ++c) {
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            const int s = c * 4 + kc;
            // Stage s has landed when at most the operations issued AFTER its four loads are outstanding (the counter retires loads and
            // stores in issue order): the loads of stages s + 1 and s + 2 and, in the first three stages of a later chunk, the previous
            // chunk's eight output stores (issued after stage s's loads: waiting for them would put a store's round trip into every
            // chunk).  Before stage 0 everything older (the row pass's stores) is waited for.
            {
                const bool last = c + 1 == (N2 >> 8);
                const int n = (kc < 2 ? 8 : kc == 2 ? (last ? 4 : 8) : (last ? 0 : 8)) + ((c > 0 && kc < 3) ? 8 : 0);
                if (n == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                else if (n == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                else if (n == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                else if (n == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
            }
            wg_barrier();                                  // stage s landed for every wave; everyone is done with stage s - 1 (and, at s = 0, with h in LDS)
            if (s + 3 < nst) issue2(s + 3);
            const char* sW = slot2(s);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8_t bf[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) bf[j] = *reinterpret_cast<const bf16x8_t*>(sW + pswz(wave * 32 + j * 16 + fr, ks * 4 + kg));
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[j], ah[kc * 2 + ks][i], acc[i][j], 0, 0, 0);
            }
        }
        // chunk complete: (+ bias, ReLU,) bf16, straight from the accumulators (a lane: 4 consecutive channels of one row, 8 bytes);
        // exactly eight stores per wave (see the waits above)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = c * PC + wave * 32 + j * 16 + kg * 4;
            float4 b2 = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (!BWD) b2 = *reinterpret_cast<const float4*>(smem + B2_OFF + n * 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = m0 + i * 16 + fr;
                float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                if constexpr (!BWD) {
                    v[0] += b2.x; v[1] += b2.y; v[2] += b2.z; v[3] += b2.w;
                    if (a.relu) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                    }
                }
                typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
                const u32x2_t w = {f2bf2(v[0], v[1]), f2bf2(v[2], v[3])};
                __builtin_amdgcn_raw_buffer_store_b64(w, rs_o2, (int)(((uint32_t)row * (uint32_t)N2 + (uint32_t)n) * 2u), 0, 0);
            }
        }
        zero_acc();
    }
}

template <bool BWD>
int panel_launch(const PanelArgs& a, void* stream)
{
    if ((uint64_t)a.R * (uint64_t)a.K1 * 2 >= 0x7fffff00ull || (uint64_t)(a.R + PM) * (uint64_t)a.N2 * 2 >= 0x7fffff00ull || a.N2 > MAX_N2) return DREG_EINVAL;   // 32-bit buffer offsets
    static const hipError_t attr = hipFuncSetAttribute((const void*)ps_panel_kernel<BWD>, hipFuncAttributeMaxDynamicSharedMemorySize, PANEL_LDS);
    if (attr != hipSuccess) return DREG_ELAUNCH;
    hipLaunchKernelGGL(ps_panel_kernel<BWD>, dim3((a.R + PM - 1) / PM), dim3(PNW * 64), PANEL_LDS, (hipStream_t)stream, a);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

}  // namespace

extern "C" int dreg_ps_panel_fwd(const void* a1, const void* w1_packed, const float* bias1, const float* residual, float* x_out,
                                 const float* gamma, const float* beta, const float* pe, void* h_out, float* stats,
                                 const void* w2_packed, const float* bias2, void* out2, int R, int K1, int N2, int relu, float eps, void* stream)
{
    if (R <= 0 || K1 <= 0 || K1 % 64 || N2 <= 0 || N2 % PC) return DREG_EINVAL;
    if (!a1 || !w1_packed || !bias1 || !residual || !x_out || !gamma || !beta || !h_out || !stats || !w2_packed || !bias2 || !out2) return DREG_EINVAL;
    PanelArgs a{};
    a.a1 = (const bf16_t*)a1; a.w1 = (const bf16_t*)w1_packed; a.w2 = (const bf16_t*)w2_packed; a.out2 = (bf16_t*)out2;
    a.R = R; a.K1 = K1; a.N2 = N2; a.relu = relu; a.eps = eps; a.gamma = gamma;
    a.bias1 = bias1; a.residual = residual; a.xout = x_out; a.beta = beta; a.pe = pe; a.hout = (bf16_t*)h_out; a.stats = stats; a.bias2 = bias2;
    return panel_launch<false>(a, stream);
}

extern "C" int dreg_ps_panel_bwd(const void* g1, const void* w1t_packed, const float* x, const float* stats, const float* gamma,
                                 const float* dx_add, const float* dx_add2, float* dx, void* dx_bf16, float* part,
                                 const void* w2t_packed, void* out2, int R, int K1, int N2, void* stream)
{
    if (R <= 0 || K1 <= 0 || K1 % 64 || (N2 != 0 && N2 != PC)) return DREG_EINVAL;
    if (!g1 || !w1t_packed || !x || !stats || !gamma || !dx || !part || (N2 && (!w2t_packed || !out2))) return DREG_EINVAL;
    PanelArgs a{};
    a.a1 = (const bf16_t*)g1; a.w1 = (const bf16_t*)w1t_packed; a.w2 = (const bf16_t*)w2t_packed; a.out2 = (bf16_t*)out2;
    a.R = R; a.K1 = K1; a.N2 = N2; a.gamma = gamma;
    a.x = x; a.st = stats; a.dx_add = dx_add; a.dx_add2 = dx_add2; a.dx = dx; a.dx_bf = (bf16_t*)dx_bf16; a.part = part;
    return panel_launch<true>(a, stream);
}
