// Iso-surface of a scalar lattice as a closed INDEXED triangle mesh (marching cubes).  Rule, order and tests: DESIGN.md §3h,
// tests/mc_restatement.py; the triangle table is derived, not transcribed (tools/make_mc_table.py -> mc_table.h).
//   values fp32 [nz, ny, nx], x fastest.  A node is inside when value > level (NaN: outside).  The edge from a node to its +x / +y / +z neighbour
//   crosses when exactly one end is inside and then owns ONE vertex; vertices ascend by owning node n = ix + nx (iy + ny iz), x- before y- before
//   z-edge; faces ascend by cell (named by its lowest node), table order inside a cell; right-hand normals point to the lower values.
//   Vertex (fp32, contraction off, / correctly rounded): t = (level - v_p) / (v_q - v_p); t not in [0, 1] or not finite -> 0.5; the coordinate along
//   the edge is origin + ((float)i + t) * spacing, the two others origin + (float)j * spacing.
// Two tile passes and a two-kernel scan, no atomics, no library scan: every launch of the same input writes the same bytes.
//   mc_count_kernel   a workgroup of 8 waves owns 8 y-rows x 8 z-planes over the whole x extent and walks x in steps of 64: each step stages
//                     9 x 9 x 65 values (the tile and its +1 halo: only + neighbours are ever read) in LDS, one lane per node along x.  A wave owns
//                     one z-plane: per row it forms the three edge flags and the cell's triangle count, ranks them inside the wave by ballot +
//                     popcount, and carries the row's running totals in registers across the x steps.  Per node ONE 32-bit word goes out:
//                     bits 0-11 the node's vertex prefix inside its row (<= 3 * 1023), 12-14 the edge flags, 15 the inside bit, 16-31 the cell's
//                     face prefix inside its row (<= 5 * 1023); per row the two totals.
//   mc_scan_rows_kernel / mc_scan_parts_kernel   exclusive prefix of the row totals in blocks of MC_SCAN_CHUNK rows, then of the block totals by one
//                     workgroup, which also writes counts = (V, F) and a stamp of the call (totals, nx, ny, nz, level) into the workspace.
//   mc_emit_kernel    the same tile walk over values and words: vertex index = row base + word prefix + rank among the node's flags; a cell's
//                     configuration and its corners' vertex indices come from the staged WORDS alone, so the counts the buffers were sized by
//                     bound every index whatever `values` holds; stores are guarded by V and F as well.
// Each value is fetched by (81 / 64) (65 / 64) = 1.29 workgroups; the repeats are neighbouring workgroups' and meet in L2 / Infinity Cache.
#include <string.h>
#include "common.h"
#include "mc_table.h"

constexpr int MC_TX = 64, MC_TY = 8, MC_TZ = 8;              // nodes per step along x (one wave), rows and planes owned by a workgroup
constexpr int MC_SX = MC_TX + 1, MC_SY = MC_TY + 1, MC_SZ = MC_TZ + 1;
constexpr int MC_BLOCK = 64 * MC_TZ;
constexpr int MC_SCAN_BLOCK = 1024, MC_SCAN_ITEMS = 4, MC_SCAN_CHUNK = MC_SCAN_BLOCK * MC_SCAN_ITEMS;
constexpr int MC_MAX_DIM = 1024;
constexpr size_t MC_MAX_NODES = (size_t)1 << 28;
constexpr int MC_STAMP = 8;                                  // uint32: V, F, nx, ny, nz, level bits, 2 spare
static_assert(3 * (MC_MAX_DIM - 1) < (1 << 12) && DREG_MC_WIDTH * (MC_MAX_DIM - 1) < (1 << 16) && DREG_MC_WIDTH < 8, "word layout");
static_assert(MC_MAX_NODES * DREG_MC_WIDTH < ((size_t)1 << 31), "F fits an int");

struct McLayout { size_t words, rowV, rowF, partV, partF, stamp, total; int rows, parts; };   // offsets in uint32 units

static inline McLayout mc_layout(int nx, int ny, int nz)
{
    McLayout l;
    const size_t n = (size_t)nx * ny * nz;
    l.rows = ny * nz;
    l.parts = (l.rows + MC_SCAN_CHUNK - 1) / MC_SCAN_CHUNK;
    l.words = 0;
    l.rowV = n;
    l.rowF = l.rowV + l.rows;
    l.partV = l.rowF + l.rows;
    l.partF = l.partV + l.parts;
    l.stamp = l.partF + l.parts;
    l.total = l.stamp + MC_STAMP;
    return l;
}

static inline bool mc_dims_ok(int nx, int ny, int nz)
{
    if (nx < 2 || ny < 2 || nz < 2 || nx > MC_MAX_DIM || ny > MC_MAX_DIM || nz > MC_MAX_DIM) return false;
    return (size_t)nx * ny * nz <= MC_MAX_NODES;
}

__device__ __forceinline__ uint32_t mc_rank(unsigned long long ballot, unsigned long long below) { return (uint32_t)__popcll(ballot & below); }

// Stage the tile of `src` for the x step at x0 (`fill` where the lattice ends).  Wave w takes the staged rows w, w + 8, ...: the row's address is
// wave-uniform, lane l loads column l (one coalesced 256-byte read per row), and the rows' 65th columns (the +x halo) go in one more read, lane j
// taking that of the wave's j-th row.
constexpr int MC_STAGE_ROWS = (MC_SZ * MC_SY + MC_TZ - 1) / MC_TZ;
template <typename T>
__device__ __forceinline__ void mc_stage(T (&s)[MC_SZ][MC_SY][MC_SX], const T* __restrict__ src, int nx, int ny, int nz, int x0, int y0, int z0, T fill)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool col = x0 + lane < nx;
#pragma unroll
    for (int k = 0; k < MC_STAGE_ROWS; ++k) {
        const int r = wave + k * MC_TZ;                      // wave-uniform
        if (r < MC_SZ * MC_SY) {
            const int sy = r % MC_SY, sz = r / MC_SY;
            const int gy = y0 + sy, gz = z0 + sz;
            T v = fill;
            if (col && gy < ny && gz < nz) v = src[((size_t)gz * ny + gy) * nx + x0 + lane];
            s[sz][sy][lane] = v;
        }
    }
    const int r = wave + lane * MC_TZ;
    if (lane < MC_STAGE_ROWS && r < MC_SZ * MC_SY) {
        const int sy = r % MC_SY, sz = r / MC_SY;
        const int gy = y0 + sy, gz = z0 + sz;
        T v = fill;
        if (x0 + MC_TX < nx && gy < ny && gz < nz) v = src[((size_t)gz * ny + gy) * nx + x0 + MC_TX];
        s[sz][sy][MC_TX] = v;
    }
}

__global__ __launch_bounds__(MC_BLOCK) void mc_count_kernel(const float* __restrict__ values, int nx, int ny, int nz, float level, uint32_t* __restrict__ words,
                                                            uint32_t* __restrict__ rowV, uint32_t* __restrict__ rowF)
{
    __shared__ float sv[MC_SZ][MC_SY][MC_SX];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int y0 = (int)blockIdx.x * MC_TY, z0 = (int)blockIdx.y * MC_TZ;
    const int z = z0 + wave;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t carryV[MC_TY], carryF[MC_TY];
#pragma unroll
    for (int ry = 0; ry < MC_TY; ++ry) carryV[ry] = carryF[ry] = 0u;
    for (int x0 = 0; x0 < nx; x0 += MC_TX) {
        __syncthreads();                                     // the previous step has been read by every wave
        mc_stage(sv, values, nx, ny, nz, x0, y0, z0, __builtin_nanf(""));      // NaN: outside
        __syncthreads();
        const int x = x0 + lane;
#pragma unroll
        for (int ry = 0; ry < MC_TY; ++ry) {
            const int y = y0 + ry;
            const bool node = x < nx && y < ny && z < nz;
            uint32_t cfg = 0;
#pragma unroll
            for (int c = 0; c < 8; ++c) cfg |= (sv[wave + (c >> 2)][ry + ((c >> 1) & 1)][lane + (c & 1)] > level ? 1u : 0u) << c;
            const bool hx = x + 1 < nx, hy = y + 1 < ny, hz = z + 1 < nz;
            const uint32_t in = cfg & 1u;
            const bool fx = node && hx && in != ((cfg >> 1) & 1u), fy = node && hy && in != ((cfg >> 2) & 1u), fz = node && hz && in != ((cfg >> 4) & 1u);
            const uint32_t nt = (node && hx && hy && hz) ? DREG_MC_NTRI[cfg] : 0u;
            const unsigned long long bx = __ballot(fx), by = __ballot(fy), bz = __ballot(fz);
            const unsigned long long t0 = __ballot(nt & 1u), t1 = __ballot(nt & 2u), t2 = __ballot(nt & 4u);
            const uint32_t pv = carryV[ry] + mc_rank(bx, below) + mc_rank(by, below) + mc_rank(bz, below);
            const uint32_t pf = carryF[ry] + mc_rank(t0, below) + 2u * mc_rank(t1, below) + 4u * mc_rank(t2, below);
            if (node) words[((size_t)z * ny + y) * nx + x] = pv | ((uint32_t)fx << 12) | ((uint32_t)fy << 13) | ((uint32_t)fz << 14) | (in << 15) | (pf << 16);
            carryV[ry] += (uint32_t)(__popcll(bx) + __popcll(by) + __popcll(bz));
            carryF[ry] += (uint32_t)(__popcll(t0) + 2 * __popcll(t1) + 4 * __popcll(t2));
        }
    }
    if (lane == 0 && z < nz) {
#pragma unroll
        for (int ry = 0; ry < MC_TY; ++ry)
            if (y0 + ry < ny) {
                rowV[(size_t)z * ny + y0 + ry] = carryV[ry];
                rowF[(size_t)z * ny + y0 + ry] = carryF[ry];
            }
    }
}

// exclusive prefix of one value per thread over a workgroup of MC_SCAN_BLOCK threads; *total = the sum.  sm: MC_SCAN_BLOCK / 64 words.
__device__ __forceinline__ uint32_t mc_block_exscan(uint32_t v, uint32_t* sm, uint32_t* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    __syncthreads();                                         // sm may still be read from the previous call
    if (lane == 63) sm[wave] = inc;
    __syncthreads();
    uint32_t base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < MC_SCAN_BLOCK / 64; ++w) {
        const uint32_t s = sm[w];
        if (w < wave) base += s;
        sum += s;
    }
    *total = sum;
    return base + inc - v;
}

// in place: a[r] -> exclusive prefix inside its chunk of MC_SCAN_CHUNK entries; part[chunk] = the chunk's sum
__global__ __launch_bounds__(MC_SCAN_BLOCK) void mc_scan_rows_kernel(uint32_t* __restrict__ rowV, uint32_t* __restrict__ rowF, int rows, uint32_t* __restrict__ partV,
                                                                     uint32_t* __restrict__ partF)
{
    __shared__ uint32_t sm[MC_SCAN_BLOCK / 64];
    const size_t first = (size_t)blockIdx.x * MC_SCAN_CHUNK + (size_t)threadIdx.x * MC_SCAN_ITEMS;
    for (int which = 0; which < 2; ++which) {
        uint32_t* a = which ? rowF : rowV;
        uint32_t v[MC_SCAN_ITEMS], mine = 0;
#pragma unroll
        for (int k = 0; k < MC_SCAN_ITEMS; ++k) {
            v[k] = first + k < (size_t)rows ? a[first + k] : 0u;
            mine += v[k];
        }
        uint32_t total;
        uint32_t run = mc_block_exscan(mine, sm, &total);
#pragma unroll
        for (int k = 0; k < MC_SCAN_ITEMS; ++k) {
            if (first + k < (size_t)rows) a[first + k] = run;
            run += v[k];
        }
        if (threadIdx.x == 0) (which ? partF : partV)[blockIdx.x] = total;
    }
}

// one workgroup: exclusive prefix of the chunk sums in place, the totals to counts and, with the call's parameters, to the stamp
__global__ __launch_bounds__(MC_SCAN_BLOCK) void mc_scan_parts_kernel(uint32_t* __restrict__ partV, uint32_t* __restrict__ partF, int parts, int nx, int ny, int nz,
                                                                      float level, uint32_t* __restrict__ stamp, int* __restrict__ counts)
{
    __shared__ uint32_t sm[MC_SCAN_BLOCK / 64];
    for (int which = 0; which < 2; ++which) {
        uint32_t* a = which ? partF : partV;
        uint32_t carry = 0;
        for (int b = 0; b < parts; b += MC_SCAN_BLOCK) {
            const int i = b + (int)threadIdx.x;
            const uint32_t v = i < parts ? a[i] : 0u;
            uint32_t total;
            const uint32_t ex = mc_block_exscan(v, sm, &total);
            if (i < parts) a[i] = carry + ex;
            carry += total;
        }
        if (threadIdx.x == 0) {
            stamp[which] = carry;
            counts[which] = (int)carry;
        }
    }
    if (threadIdx.x == 0) {
        stamp[2] = (uint32_t)nx; stamp[3] = (uint32_t)ny; stamp[4] = (uint32_t)nz; stamp[5] = __float_as_uint(level);
        stamp[6] = stamp[7] = 0u;
    }
}

struct McGrid { float o[3], s[3]; };

__device__ __forceinline__ float mc_cross_t(float level, float vp, float vq)
{
    const float t = (level - vp) / (vq - vp);
    return (t >= 0.f && t <= 1.f) ? t : 0.5f;                // NaN and +-inf fail the comparison
}

__global__ __launch_bounds__(MC_BLOCK) void mc_emit_kernel(const float* __restrict__ values, int nx, int ny, int nz, float level, McGrid g,
                                                           const uint32_t* __restrict__ words, const uint32_t* __restrict__ rowV, const uint32_t* __restrict__ rowF,
                                                           const uint32_t* __restrict__ partV, const uint32_t* __restrict__ partF, float* __restrict__ verts,
                                                           int* __restrict__ faces, uint32_t V, uint32_t F)
{
    __shared__ float sv[MC_SZ][MC_SY][MC_SX];
    __shared__ uint32_t sw[MC_SZ][MC_SY][MC_SX];
    __shared__ uint32_t baseV[MC_SZ][MC_SY], baseF[MC_SZ][MC_SY];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int y0 = (int)blockIdx.x * MC_TY, z0 = (int)blockIdx.y * MC_TZ;
    const int z = z0 + wave;
    if (threadIdx.x < MC_SZ * MC_SY) {                       // global prefix of every staged row: chunk prefix + prefix inside the chunk
        const int sy = threadIdx.x % MC_SY, sz = threadIdx.x / MC_SY;
        uint32_t bv = 0, bf = 0;
        if (y0 + sy < ny && z0 + sz < nz) {
            const size_t r = (size_t)(z0 + sz) * ny + (y0 + sy);
            bv = rowV[r] + partV[r / MC_SCAN_CHUNK];
            bf = rowF[r] + partF[r / MC_SCAN_CHUNK];
        }
        baseV[sz][sy] = bv;
        baseF[sz][sy] = bf;
    }
    for (int x0 = 0; x0 < nx; x0 += MC_TX) {
        __syncthreads();
        mc_stage(sv, values, nx, ny, nz, x0, y0, z0, __builtin_nanf(""));
        mc_stage(sw, words, nx, ny, nz, x0, y0, z0, 0u);
        __syncthreads();
        const int x = x0 + lane;
#pragma unroll 1
        for (int ry = 0; ry < MC_TY; ++ry) {
            const int y = y0 + ry;
            if (!(x < nx && y < ny && z < nz)) continue;
            const uint32_t w = sw[wave][ry][lane];
            const uint32_t flags = (w >> 12) & 7u;
            if (flags) {
                uint32_t vi = baseV[wave][ry] + (w & 0xfffu);
                const float vp = sv[wave][ry][lane];
                const float px = g.o[0] + (float)x * g.s[0], py = g.o[1] + (float)y * g.s[1], pz = g.o[2] + (float)z * g.s[2];
                if (flags & 1u) {
                    const float t = mc_cross_t(level, vp, sv[wave][ry][lane + 1]);
                    if (vi < V) { verts[3 * (size_t)vi] = g.o[0] + ((float)x + t) * g.s[0]; verts[3 * (size_t)vi + 1] = py; verts[3 * (size_t)vi + 2] = pz; }
                    ++vi;
                }
                if (flags & 2u) {
                    const float t = mc_cross_t(level, vp, sv[wave][ry + 1][lane]);
                    if (vi < V) { verts[3 * (size_t)vi] = px; verts[3 * (size_t)vi + 1] = g.o[1] + ((float)y + t) * g.s[1]; verts[3 * (size_t)vi + 2] = pz; }
                    ++vi;
                }
                if (flags & 4u) {
                    const float t = mc_cross_t(level, vp, sv[wave + 1][ry][lane]);
                    if (vi < V) { verts[3 * (size_t)vi] = px; verts[3 * (size_t)vi + 1] = py; verts[3 * (size_t)vi + 2] = g.o[2] + ((float)z + t) * g.s[2]; }
                }
            }
            if (!(x + 1 < nx && y + 1 < ny && z + 1 < nz)) continue;
            uint32_t cfg = 0;
#pragma unroll
            for (int c = 0; c < 8; ++c) cfg |= ((sw[wave + (c >> 2)][ry + ((c >> 1) & 1)][lane + (c & 1)] >> 15) & 1u) << c;
            const uint32_t nt = DREG_MC_NTRI[cfg];
            const uint32_t fi = baseF[wave][ry] + (w >> 16);
            for (uint32_t k = 0; k < nt; ++k) {
                if (fi + k >= F) break;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int e = DREG_MC_TRI[cfg][3 * k + j];
                    const int axis = e >> 2, a = e & 1, b = (e >> 1) & 1;
                    const int dx = axis == 0 ? 0 : a, dy = axis == 0 ? a : (axis == 1 ? 0 : b), dz = axis == 2 ? 0 : b;
                    const uint32_t wq = sw[wave + dz][ry + dy][lane + dx];
                    const uint32_t fl = (wq >> 12) & 7u;
                    const uint32_t rank = axis == 0 ? 0u : (axis == 1 ? (fl & 1u) : (fl & 1u) + ((fl >> 1) & 1u));
                    faces[3 * (size_t)(fi + k) + j] = (int)(baseV[wave + dz][ry + dy] + (wq & 0xfffu) + rank);
                }
            }
        }
    }
}

extern "C" {

int dreg_mc_table(signed char* tris, int* width)
{
    if (!width) return DREG_EINVAL;
    *width = DREG_MC_WIDTH;
    if (tris)
        for (int c = 0; c < 256; ++c)
            for (int k = 0; k < 3 * DREG_MC_WIDTH; ++k) tris[c * 3 * DREG_MC_WIDTH + k] = DREG_MC_TRI[c][k];
    return DREG_OK;
}

size_t dreg_mc_workspace_bytes(int nx, int ny, int nz)
{
    if (!mc_dims_ok(nx, ny, nz)) return 0;
    return mc_layout(nx, ny, nz).total * sizeof(uint32_t);
}

int dreg_mc_count(const float* values, int nx, int ny, int nz, float level, void* workspace, size_t workspace_bytes, int* counts, void* stream)
{
    if (!values || !workspace || !counts || !mc_dims_ok(nx, ny, nz)) return DREG_EINVAL;
    if (workspace_bytes < dreg_mc_workspace_bytes(nx, ny, nz) || ((uintptr_t)workspace & 3)) return DREG_EINVAL;
    const McLayout l = mc_layout(nx, ny, nz);
    uint32_t* ws = (uint32_t*)workspace;
    const dim3 grid((ny + MC_TY - 1) / MC_TY, (nz + MC_TZ - 1) / MC_TZ);
    hipLaunchKernelGGL(mc_count_kernel, grid, dim3(MC_BLOCK), 0, (hipStream_t)stream, values, nx, ny, nz, level, ws + l.words, ws + l.rowV, ws + l.rowF);
    hipLaunchKernelGGL(mc_scan_rows_kernel, dim3(l.parts), dim3(MC_SCAN_BLOCK), 0, (hipStream_t)stream, ws + l.rowV, ws + l.rowF, l.rows, ws + l.partV, ws + l.partF);
    hipLaunchKernelGGL(mc_scan_parts_kernel, dim3(1), dim3(MC_SCAN_BLOCK), 0, (hipStream_t)stream, ws + l.partV, ws + l.partF, l.parts, nx, ny, nz, level, ws + l.stamp,
                       counts);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

int dreg_mc_emit(const float* values, int nx, int ny, int nz, float level, const float* origin, const float* spacing, const void* workspace,
                 size_t workspace_bytes, float* verts, int* faces, int V, int F, void* stream)
{
    if (!values || !origin || !spacing || !workspace || V < 0 || F < 0 || !mc_dims_ok(nx, ny, nz)) return DREG_EINVAL;
    if ((V > 0 && !verts) || (F > 0 && !faces)) return DREG_EINVAL;
    if (workspace_bytes < dreg_mc_workspace_bytes(nx, ny, nz) || ((uintptr_t)workspace & 3)) return DREG_EINVAL;
    const McLayout l = mc_layout(nx, ny, nz);
    const uint32_t* ws = (const uint32_t*)workspace;
    // the stamp the count call left: V, F and the call's parameters.  The caller has read `counts` already, so the stream is drained and this
    // 32-byte read waits for nothing.
    uint32_t stamp[MC_STAMP];
    if (hipMemcpyAsync(stamp, ws + l.stamp, sizeof(stamp), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess) return DREG_ELAUNCH;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return DREG_ELAUNCH;
    uint32_t lbits;
    memcpy(&lbits, &level, sizeof(lbits));
    if (stamp[0] != (uint32_t)V || stamp[1] != (uint32_t)F || stamp[2] != (uint32_t)nx || stamp[3] != (uint32_t)ny || stamp[4] != (uint32_t)nz || stamp[5] != lbits)
        return DREG_EINVAL;
    if (V == 0 && F == 0) return DREG_OK;
    McGrid g;
    for (int c = 0; c < 3; ++c) { g.o[c] = origin[c]; g.s[c] = spacing[c]; }
    const dim3 grid((ny + MC_TY - 1) / MC_TY, (nz + MC_TZ - 1) / MC_TZ);
    hipLaunchKernelGGL(mc_emit_kernel, grid, dim3(MC_BLOCK), 0, (hipStream_t)stream, values, nx, ny, nz, level, g, ws + l.words, ws + l.rowV, ws + l.rowF, ws + l.partV,
                       ws + l.partF, verts, faces, (uint32_t)V, (uint32_t)F);
    DREG_LAUNCH_CHECK();
    return DREG_OK;
}

}  // extern "C"
