// Streaming 1x1x1 (pointwise) convolution, bf16, gfx950:   out[m, :] = bf16( [relu]( in[m, :] . W^T [+ bias] [+ addend[m, :]] ) )
//
// The dense 1^3 stride-1 convolutions of ResNet layers 1 / 2 move bytes (K = 64..256: 0.1-0.5 FLOP per byte).  On the implicit GEMM
// (conv.hip) a workgroup owns one tile: it loads, multiplies, round-trips its accumulators through LDS and stores, one phase after
// the other.  Here a workgroup WALKS a contiguous range of 128-row chunks (the BatchNorm chunk) in 64-row tiles:
//   * its weight slice (BN output channels x CIN) lives in REGISTERS for the whole walk — wave w owns channels w*BN/4 .. of all 64 rows;
//   * the input rows of tile t + 1 (and its addend rows) are requested, direct-to-LDS and 16 bytes per lane, BEFORE tile t's MFMAs
//     and stores: a workgroup's loads overlap its own stores and those of the other workgroups of its CU;
//   * the addend tile lands in the LDS buffer the outputs are staged in: a lane adds its 4 channels in place (fp32, one rounding) and
//     the tile leaves as whole contiguous rows, 16 bytes per lane.
// Bit-identical to conv_igemm_glds_kernel: mfma_f32_16x16x32_bf16 with the weights as the first operand and the same k-slot layout
// (lane l: row / channel l & 15, K elements 32 kk + 8 (l >> 4) .. + 7), one in-order chain over kk per accumulator, and the epilogue's
// order bias, addend, ReLU in fp32.  The BatchNorm chunk sums are those of dreg_conv3d_igemm_bnstats (canonical bracketing, see there):
// rows q and q + 64 of a chunk are the same lane's value in the chunk's two tiles, rows j, j + 16, j + 32, j + 48 its four MFMA row
// tiles, and the in-order sum over j = 0..15 runs along the 16 lanes of a DPP row.
// No cross-workgroup communication, no atomics, no persistent state.
#include "common.h"
#include "../../include/dreg_nerf.h"   // signature check of every entry point defined here

// Workgroup barrier over LDS traffic only.  __syncthreads() also drains vmcnt — the direct-to-LDS requests of the NEXT tile, which must stay
// in flight across this tile's MFMAs and stores; what a barrier here has to order is named at its call (a counted vmcnt wait in front of the
// first one of an iteration: this tile's own pieces).
__device__ __forceinline__ void wg_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// The LDS traffic of the addend / output image is written as instructions: the compiler cannot tell these accesses from the image a
// direct-to-LDS request is filling (the other buffer, or none) and would put s_waitcnt vmcnt(0) in front of each — the next tile's requests again.
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
// (reads come with their wait in ONE statement: the compiler takes an asm's outputs for valid the moment the statement ends)
__device__ __forceinline__ void lds_rd64x4(const uint32_t (&a)[4], u32x2_t (&v)[4]) {
    asm volatile("ds_read_b64 %0, %4\n\tds_read_b64 %1, %5\n\tds_read_b64 %2, %6\n\tds_read_b64 %3, %7\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]) : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_rd128x2(uint32_t a, u32x4_t& v0, u32x4_t& v1) {
    asm volatile("ds_read_b128 %0, %2 offset:%3\n\tds_read_b128 %1, %2 offset:%4\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v0), "=&v"(v1) : "v"(a), "n"(OFF), "n"(OFF + 4096) : "memory");
}
__device__ __forceinline__ void lds_wr64(uint32_t a, u32x2_t v) { asm volatile("ds_write_b64 %0, %1" ::"v"(a), "v"(v) : "memory"); }
__device__ __forceinline__ void lds_wr128(uint32_t a, f32x4_t v) { asm volatile("ds_write_b128 %0, %1" ::"v"(a), "v"(v) : "memory"); }

// lane l of a 16-lane DPP row receives lane l - 1's value, lane 0 receives 0
__device__ __forceinline__ float dpp_shr1(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, true)); }

template <int CIN, int BN, bool STATS>
__global__ __launch_bounds__(256, 2) void conv1_stream_kernel(
    const bf16_t* __restrict__ in, const bf16_t* __restrict__ wt, bf16_t* out, const float* __restrict__ bias, const bf16_t* addend,
    uint32_t M, int Cout, int Kpad, int relu, uint32_t in_bytes, uint32_t out_bytes, uint32_t nchunks, float* __restrict__ bn_part)
{
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    constexpr int TN = BN / 64, KK = CIN / 32, RB = BN * 2;             // 16-channel tiles per wave, 32-element K groups, bytes per staged output row
    constexpr int SWM = (BN / 8 < 16 ? BN / 8 : 16) - 1;                 // the output tile's 16-byte granules are XOR-ed with row & SWM
    constexpr int IN_BYTES = 64 * CIN * 2, OB_BYTES = 64 * RB;
    constexpr int PA = CIN / 32, PO = BN / 32;                           // 1 KiB direct-to-LDS pieces per wave and tile: input, addend
    constexpr uint32_t OOB = 0x7fffff00u;
    extern __shared__ __attribute__((aligned(16))) char smem[];         // [2][IN_BYTES] input stages, [1 or 2][OB_BYTES] output tiles (2 with an addend: they arrive in them)

    const bool has_add = addend != nullptr;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int n0 = blockIdx.y * BN;
    const uint32_t c_begin = (uint32_t)((uint64_t)blockIdx.x * nchunks / gridDim.x);
    const uint32_t c_end = (uint32_t)((uint64_t)(blockIdx.x + 1) * nchunks / gridDim.x);
    const int ntiles = 2 * (int)(c_end - c_begin);
    if (ntiles <= 0) return;

    const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc((void*)in, 0, in_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_add = __builtin_amdgcn_make_buffer_rsrc((void*)(has_add ? addend : out), 0, out_bytes, 0x00020000);

    // input stage: [CIN/64 K blocks][64 rows][128 B], the implicit GEMM's image (swizzle applied on the source side: physical slot s of row r
    // holds logical granule s ^ ((r >> 1) & 7)).  Piece p = K block p >> 3, rows 8 (p & 7) .. + 7.
    uint32_t aoff[PA];
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        const int p = wave * PA + i, kb = p >> 3, r = (p & 7) * 8 + (lane >> 3);
        const int gl = (lane & 7) ^ ((r >> 1) & 7);
        aoff[i] = (uint32_t)(r * CIN * 2 + kb * 128 + gl * 16);
    }
    // addend / output tile: [64 rows][BN] bf16, linear per piece; physical granule g of row r holds logical granule g ^ (r & SWM)
    uint32_t ooff[PO];
#pragma unroll
    for (int i = 0; i < PO; ++i) {
        const int q = (wave * PO + i) * 1024 + lane * 16, r = q / RB, lg = ((q % RB) >> 4) ^ (r & SWM);
        ooff[i] = (uint32_t)(r * Cout * 2 + (n0 + lg * 8) * 2);
    }
#pragma unroll
    for (int i = 0; i < PA; ++i) asm volatile("" : "+v"(aoff[i]));
#pragma unroll
    for (int i = 0; i < PO; ++i) asm volatile("" : "+v"(ooff[i]));

    auto issue = [&](int ti, int buf) {
        const uint32_t m0 = (2u * c_begin + (uint32_t)ti) * 64u;
        const int rem = m0 < M ? (int)(M - m0 < 64u ? M - m0 : 64u) : 0;        // valid rows of the tile
        char* sA = smem + buf * IN_BYTES + wave * PA * 1024;
        const uint32_t soA = m0 * (uint32_t)(CIN * 2);
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const int r = ((wave * PA + i) & 7) * 8 + (lane >> 3);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_in, (lds_ptr_t)(sA + i * 1024), 16, (int)(r < rem ? aoff[i] : OOB), (int)soA, 0, 0);
        }
        if (has_add) {
            char* sO = smem + 2 * IN_BYTES + buf * OB_BYTES + wave * PO * 1024;
            const uint32_t soO = m0 * (uint32_t)(Cout * 2);
#pragma unroll
            for (int i = 0; i < PO; ++i) {
                const int r = ((wave * PO + i) * 1024 + lane * 16) / RB;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_add, (lds_ptr_t)(sO + i * 1024), 16, (int)(r < rem ? ooff[i] : OOB), (int)soO, 0, 0);
            }
        }
    };

    // tile 0 is on its way while the weights and the bias arrive
    issue(0, 0);
    const int fr = lane & 15, kg = lane >> 4;
    bf16x8_t bw[TN][KK];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int kk = 0; kk < KK; ++kk)
            bw[j][kk] = *reinterpret_cast<const bf16x8_t*>(wt + (size_t)(n0 + wave * (BN / 4) + j * 16 + fr) * Kpad + kk * 32 + kg * 8);
    float b4[TN][4];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) b4[j][r] = bias ? bias[n0 + wave * (BN / 4) + j * 16 + kg * 4 + r] : 0.f;

    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    u32x2_t keep[STATS ? TN : 1][4];               // STATS: the rounded outputs of a chunk's first tile
#pragma unroll
    for (int j = 0; j < (STATS ? TN : 1); ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) keep[j][i] = (u32x2_t){0u, 0u};

    for (int ti = 0; ti < ntiles; ++ti) {
        const int cur = ti & 1;
        // tile ti + 1 is requested before this tile's MFMAs and stores; its pieces are the youngest loads of the wave, and loads retire in
        // order among themselves, so a counter at or below their number means tile ti has landed (whatever the stores in between do)
        if (ti + 1 < ntiles) {
            issue(ti + 1, cur ^ 1);
            if (has_add) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PA + PO) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PA) : "memory");
        } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        wg_barrier();

        f32x4_t acc[4][TN];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        const char* sA = smem + cur * IN_BYTES;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            bf16x8_t af[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = i * 16 + fr, slot = (kk & 1) * 4 + kg;
                af[i] = *reinterpret_cast<const bf16x8_t*>(sA + (kk >> 1) * 8192 + row * 128 + ((slot ^ ((row >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[j][kk], af[i], acc[i][j], 0, 0, 0);   // C^T: a lane holds 4 consecutive channels of one row
        }

        // epilogue: lane (rl = lane & 15, gq = lane >> 4) holds rows 16 i + rl, channels wave * BN/4 + 16 j + 4 gq .. + 3
        const uint32_t oO = lds0 + 2 * IN_BYTES + (has_add ? cur : 0) * OB_BYTES;      // LDS address of this tile's addend / output image
        const bool second = STATS && (ti & 1) != 0;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int lg = wave * (BN / 32) + 2 * j + (kg >> 1);
            uint32_t pa[4];
            u32x2_t ad[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = i * 16 + fr;
                pa[i] = oO + row * RB + ((lg ^ (row & SWM)) << 4) + (kg & 1) * 8;
            }
            if (has_add) lds_rd64x4(pa, ad);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                if (bias) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] += b4[j][r];
                }
                if (has_add) {
                    v[0] += __uint_as_float(ad[i][0] << 16); v[1] += __uint_as_float(ad[i][0] & 0xffff0000u);
                    v[2] += __uint_as_float(ad[i][1] << 16); v[3] += __uint_as_float(ad[i][1] & 0xffff0000u);
                }
                if (relu) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
                }
                const u32x2_t w = {f2bf2(v[0], v[1]), f2bf2(v[2], v[3])};
                lds_wr64(pa[i], w);
                if constexpr (STATS) { if (!second) keep[j][i] = w; }
            }
        }
        wg_barrier();

        // the tile leaves as whole rows: a wave-instruction reads 1 KiB of the staged tile and writes 1024 / RB complete output rows
        {
            const uint32_t m0 = (2u * c_begin + (uint32_t)ti) * 64u;
            constexpr int NIT = OB_BYTES / 4096;
            u32x4_t v[NIT];
            static_assert(NIT == 2 || NIT == 4 || NIT == 8, "staged tile: pairs of 4 KiB read phases");
            lds_rd128x2<0>(oO + t * 16, v[0], v[1]);
            if constexpr (NIT >= 4) lds_rd128x2<8192>(oO + t * 16, v[2], v[3]);
            if constexpr (NIT >= 8) { lds_rd128x2<16384>(oO + t * 16, v[4], v[5]); lds_rd128x2<24576>(oO + t * 16, v[6], v[7]); }
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int q = it * 4096 + t * 16, r = q / RB, lg = ((q % RB) >> 4) ^ (r & SWM);
                if (m0 + (uint32_t)r < M) __builtin_nontemporal_store(v[it], reinterpret_cast<u32x4_t*>(out + (size_t)(m0 + r) * Cout + n0 + lg * 8));
            }
        }

        if (second) {
            // BatchNorm sums of the chunk (the accumulators are dead by now): a lane's kept value of the first tile is row q, its staged value of
            // the second row q + 64; its four row tiles are the classes j, j + 16, j + 32, j + 48 of the canonical bracket
            float s1[TN][4], s2[TN][4], a1[TN][4], a2[TN][4];
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int lg = wave * (BN / 32) + 2 * j + (kg >> 1);
                float c1[4][4], c2[4][4];
                u32x2_t kb[4];
                uint32_t pa[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = i * 16 + fr;
                    pa[i] = oO + row * RB + ((lg ^ (row & SWM)) << 4) + (kg & 1) * 8;
                }
                lds_rd64x4(pa, kb);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const u32x2_t ka = keep[j][i];
                    const float xa[4] = {__uint_as_float(ka[0] << 16), __uint_as_float(ka[0] & 0xffff0000u), __uint_as_float(ka[1] << 16), __uint_as_float(ka[1] & 0xffff0000u)};
                    const float xb[4] = {__uint_as_float(kb[i][0] << 16), __uint_as_float(kb[i][0] & 0xffff0000u), __uint_as_float(kb[i][1] << 16), __uint_as_float(kb[i][1] & 0xffff0000u)};
#pragma unroll
                    for (int r = 0; r < 4; ++r) { c1[i][r] = xa[r] + xb[r]; c2[i][r] = xa[r] * xa[r] + xb[r] * xb[r]; }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s1[j][r] = (c1[0][r] + c1[2][r]) + (c1[1][r] + c1[3][r]);
                    s2[j][r] = (c2[0][r] + c2[2][r]) + (c2[1][r] + c2[3][r]);
                }
            }
            // sum over j = 0..15 of the lanes' brackets, in order (a = 0; a += t[0]; ... a += t[15]): the 16 lanes of a DPP row hold t[0..15] of the same
            // channels; step k of s <- shift_right_1(s) + t leaves the first k + 1 lanes with their final prefix, lane 15 with the sum after step 15
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) { a1[j][r] = 0.f + s1[j][r]; a2[j][r] = 0.f + s2[j][r]; }
#pragma unroll
            for (int k = 1; k < 16; ++k)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) { a1[j][r] = dpp_shr1(a1[j][r]) + s1[j][r]; a2[j][r] = dpp_shr1(a2[j][r]) + s2[j][r]; }
            if (fr == 15) {
                const size_t chunk = (size_t)c_begin + (size_t)(ti >> 1);
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    float* o = bn_part + (chunk * Cout + n0 + wave * (BN / 4) + j * 16 + kg * 4) * 2;
                    *reinterpret_cast<float4*>(o) = make_float4(a1[j][0], a2[j][0], a1[j][1], a2[j][1]);
                    *reinterpret_cast<float4*>(o + 4) = make_float4(a1[j][2], a2[j][2], a1[j][3], a2[j][3]);
                }
            }
        }
        // the next iteration requests tile ti + 2 into the buffers this one read
        if (has_add) wg_barrier();
    }
}

// ------------------------------------------------------------------------------------------------ host
// the (Cin, Cout) pairs that have an instantiation: output channels per workgroup (0 = none)
static int pw_bn(int Cin, int Cout)
{
    if (Cin == 64) return Cout == 64 ? 64 : (Cout % 128 == 0 ? 128 : 0);
    if (Cin == 128) return Cout % 128 == 0 ? 128 : 0;
    if (Cin == 256) return Cout == 64 ? 64 : (Cout % 128 == 0 ? 128 : 0);
    return 0;
}
static size_t pw_lds(int Cin, int bn, bool two_tiles) { return (size_t)2 * 64 * Cin * 2 + (size_t)(two_tiles ? 2 : 1) * 64 * bn * 2; }

template <int CIN, int BN, bool STATS>
static void pw_launch1(dim3 grid, size_t lds, hipStream_t st, const void* in, const void* wt, void* out, const float* bias, const void* addend,
                      uint32_t M, int Cout, int Kpad, int relu, uint32_t nchunks, float* bn_part)
{
    if (lds > 65536) (void)hipFuncSetAttribute((const void*)conv1_stream_kernel<CIN, BN, STATS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((conv1_stream_kernel<CIN, BN, STATS>), grid, dim3(256), lds, st, (const bf16_t*)in, (const bf16_t*)wt, (bf16_t*)out, bias, (const bf16_t*)addend,
                       M, Cout, Kpad, relu, (uint32_t)((uint64_t)M * CIN * 2), (uint32_t)((uint64_t)M * Cout * 2), nchunks, bn_part);
}

template <int CIN, int BN>
static void pw_launch(dim3 grid, size_t lds, hipStream_t st, const void* in, const void* wt, void* out, const float* bias, const void* addend,
                      uint32_t M, int Cout, int Kpad, int relu, uint32_t nchunks, float* bn_part)
{
    if (bn_part) pw_launch1<CIN, BN, true>(grid, lds, st, in, wt, out, bias, addend, M, Cout, Kpad, relu, nchunks, bn_part);
    else pw_launch1<CIN, BN, false>(grid, lds, st, in, wt, out, bias, addend, M, Cout, Kpad, relu, nchunks, nullptr);
}

static int pw_run(const void* in, const void* wt, void* out, const float* bias, const void* addend, uint32_t M, int Cin, int Cout, int relu,
                  float* bn_part, int max_blocks, hipStream_t st)
{
    const int bn = pw_bn(Cin, Cout);
    if (!bn) return DREG_EINVAL;
    if (M == 0) return DREG_OK;
    const size_t lds = pw_lds(Cin, bn, addend != nullptr);
    const uint32_t nchunks = (M + 127) / 128;
    const int slices = Cout / bn;
    // a few workgroups per CU (LDS decides how many), each walking a contiguous range of chunks
    int per_cu = (int)(163840 / lds);
    per_cu = per_cu > 4 ? 4 : (per_cu < 1 ? 1 : per_cu);
    uint32_t nblk = (uint32_t)(256 * per_cu / slices);
    if (max_blocks > 0) nblk = (uint32_t)max_blocks;
    if (nblk > nchunks) nblk = nchunks;
    if (nblk < 1) nblk = 1;
    const dim3 grid(nblk, slices);
    const int Kpad = dreg_conv3d_kpad(1, Cin, 0);
#define PW_CASE(C, N) if (Cin == C && bn == N) pw_launch<C, N>(grid, lds, st, in, wt, out, bias, addend, M, Cout, Kpad, relu, nchunks, bn_part); else
    PW_CASE(64, 64) PW_CASE(64, 128) PW_CASE(128, 128) PW_CASE(256, 64) PW_CASE(256, 128) return DREG_EINVAL;
#undef PW_CASE
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

// Which launches take the streaming kernel: every shape of tools/bench_pointwise.py that it runs faster by more than the repeat-to-repeat spread
// (profiles/pw_stream_by_shape.txt) — all instantiations from 32^3 voxels per grid on, and at 16^3 the two 512-channel outputs measured there
// (128 -> 512, 256 -> 512).  Like the halo kernel's rule it does not depend on how many grids share the launch.
static bool pw_faster(long V, int Cin, int Cout)
{
    if (V >= 32 * 32 * 32) return true;
    return V >= 16 * 16 * 16 && Cout == 512 && (Cin == 128 || Cin == 256);
}

extern "C" {

// output channels per workgroup of the instantiation conv1_stream_kernel<Cin, BN, ...> that serves (Cin, Cout); 0 = none (profiler labels)
int dreg_conv1_stream_variant(int Cin, int Cout) { return pw_bn(Cin, Cout); }

// Can the streaming kernel run this launch?  Dense rows (nrows == 0), 1^3 taps, stride 1, no padding, bf16 in and out, ReLU 0 / 1, a
// same-size addend (or none), a (Cin, Cout) pair with an instantiation and every operand within the 2 GiB reach of a buffer descriptor.
int dreg_conv1_stream_supported(int B, int D, int H, int W, int Cin, int Cout, int ksz, int stride, int pad, int relu,
                                int has_addend, int add_same, int dtype, int nrows)
{
    if (dtype != 0 || nrows != 0 || ksz != 1 || stride != 1 || pad != 0 || !(relu == 0 || relu == 1)) return 0;
    if (has_addend && !add_same) return 0;
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || !pw_bn(Cin, Cout)) return 0;
    const uint64_t M = (uint64_t)B * D * H * W;
    if (M * (uint64_t)Cin * 2 >= 0x7fffff00ull || M * (uint64_t)Cout * 2 >= 0x7fffff00ull) return 0;
    return 1;
}
// ... and is it the faster launch (the executor's rule)?
int dreg_conv1_stream_use(int B, int D, int H, int W, int Cin, int Cout, int ksz, int stride, int pad, int relu,
                          int has_addend, int add_same, int dtype, int nrows)
{
    if (!dreg_conv1_stream_supported(B, D, H, W, Cin, Cout, ksz, stride, pad, relu, has_addend, add_same, dtype, nrows)) return 0;
    return pw_faster((long)D * H * W, Cin, Cout) ? 1 : 0;
}

// The arguments of dreg_conv3d_igemm_ws and its result, bit for bit; launches dreg_conv1_stream_supported refuses run there.
// max_blocks: 0 = automatic, else the number of workgroups per channel slice (tests: few workgroups walk many tiles).
int dreg_conv1_stream(const void* in, const void* wt_packed, void* out, const float* bias, const void* addend,
                      int B, int Di, int Hi, int Wi, int Cin, int Do, int Ho, int Wo, int Cout,
                      int ksz, int stride, int pad, int transposed, int relu, int Da, int Ha, int Wa, int add_same,
                      int dtype, int out_f32, void* workspace, size_t workspace_bytes, void* stream, int max_blocks)
{
    const bool same = !addend || (add_same && Da == Do && Ha == Ho && Wa == Wo);
    if (out_f32 || !same || Di != Do || Hi != Ho || Wi != Wo ||
        !dreg_conv1_stream_supported(B, Do, Ho, Wo, Cin, Cout, ksz, stride, pad, relu, addend != nullptr, add_same, dtype, 0))
        return dreg_conv3d_igemm_ws(in, wt_packed, out, bias, addend, B, Di, Hi, Wi, Cin, Do, Ho, Wo, Cout, ksz, stride, pad, transposed, relu,
                                    Da, Ha, Wa, add_same, dtype, out_f32, workspace, workspace_bytes, stream);
    (void)transposed;                              // a 1^3 stride-1 data gradient is the same product over its own pack
    return pw_run(in, wt_packed, out, bias, addend, (uint32_t)((uint64_t)B * Do * Ho * Wo), Cin, Cout, relu, nullptr, max_blocks, (hipStream_t)stream);
}

// The arguments of dreg_conv3d_igemm_bnstats, its output and its chunk sums, bit for bit: bn_partial [B][V / 128][Cout][2] and
// *rows_per_chunk = 128 when V % 128 == 0, else *rows_per_chunk = 0 and nothing written there.
int dreg_conv1_stream_bnstats(const void* in, const void* wt_packed, void* out, const float* bias, const void* addend,
                              int B, int Di, int Hi, int Wi, int Cin, int Do, int Ho, int Wo, int Cout,
                              int ksz, int stride, int pad, int relu, int Da, int Ha, int Wa, int add_same,
                              void* workspace, size_t workspace_bytes, float* bn_partial, int* rows_per_chunk, void* stream, int max_blocks)
{
    if (!rows_per_chunk) return DREG_EINVAL;
    const bool same = !addend || (add_same && Da == Do && Ha == Ho && Wa == Wo);
    if (!same || Di != Do || Hi != Ho || Wi != Wo ||
        !dreg_conv1_stream_supported(B, Do, Ho, Wo, Cin, Cout, ksz, stride, pad, relu, addend != nullptr, add_same, 0, 0))
        return dreg_conv3d_igemm_bnstats(in, wt_packed, out, bias, addend, B, Di, Hi, Wi, Cin, Do, Ho, Wo, Cout, ksz, stride, pad, relu,
                                         Da, Ha, Wa, add_same, workspace, workspace_bytes, bn_partial, rows_per_chunk, stream);
    *rows_per_chunk = 0;
    const long V = (long)Do * Ho * Wo;
    const bool emit = bn_partial && V % 128 == 0;
    const int rc = pw_run(in, wt_packed, out, bias, addend, (uint32_t)((uint64_t)B * V), Cin, Cout, relu, emit ? bn_partial : nullptr, max_blocks, (hipStream_t)stream);
    if (rc == DREG_OK && emit) *rows_per_chunk = 128;
    return rc;
}

}   // extern "C"
