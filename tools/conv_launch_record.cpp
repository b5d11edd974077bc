// Host-only launch recorder for csrc/conv.hip (no GPU needed): a stand-alone program that links a checkout's objects and defines the HIP launch entry
// points itself, so every C-ABI call of a shape sweep prints what it WOULD launch — kernel symbol, grid, block, dynamic LDS and every kernel argument
// (the ConvGeom as a hash) — plus its return code and out arguments.  Two checkouts whose logs are byte-identical launch the same things; with the
// -DDREG_PROBE=1 objects the sweep is repeated under every kernel-variant knob, the stamped / "wrong results" measurement forms included.
//   R=<checkout>; hipcc --offload-arch=gfx950 -std=c++17 -I$R/include -c tools/conv_launch_record.cpp -o rec.o
//   hipcc --offload-arch=gfx950 -rdynamic rec.o $(ls $R/dreg_nerf_amd/csrc/*.o | grep -v probe) -ldl -o rec && ./rec out.log
//   probe build: add -DPROBE -DDREG_PROBE=1 to the first line and link $R/dreg_nerf_amd/csrc/*.probe.o instead.   (profiles/conv_dispatch_refactor.txt, section 3)
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <cstdio>
#include <cstring>
#include <cstdint>
#include <string>
#include "dreg_nerf.h"
#ifdef PROBE
#include "dreg_nerf_probe.h"
#endif
static FILE* out = stdout;
static std::string kname(const void* f) {
    Dl_info i; if (dladdr(f, &i) && i.dli_sname) return i.dli_sname; return "?";
}
// argument sizes per kernel family (bytes), by name fragment
static const int* sizes(const std::string& n, int& cnt) {
    static const int igl[] = {8,8,8,8,8,88,4,4,4,4,4,4,4,4,8,4,4,4,8};
    static const int ig[] = {8,8,8,8,8,88,4,4,4,4,4,4,8,8,4,8};
    static const int wg[] = {8,8,8,88,4,4,8};
    static const int wgl[] = {8,8,8,88,4,4,4,4,4,4,8,4,8,4};
    static const int sk[] = {8,8,8,8,8,4,4,4};
    static const int rd[] = {48};
    if (n.find("conv_igemm_glds_kernel") != std::string::npos) { cnt = 19; return igl; }
    if (n.find("conv_igemm_kernel") != std::string::npos) { cnt = 16; return ig; }
    if (n.find("conv_wgrad_glds_kernel") != std::string::npos) { cnt = 14; return wgl; }
    if (n.find("conv_wgrad_kernel") != std::string::npos) { cnt = 7; return wg; }
    if (n.find("splitk_reduce_kernel") != std::string::npos) { cnt = 8; return sk; }
    if (n.find("wgrad_reduce_kernel") != std::string::npos) { cnt = 1; return rd; }
    cnt = 0; return nullptr;
}
extern "C" hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void** args, size_t shmem, hipStream_t) {
    std::string n = kname(f);
    fprintf(out, "  launch %s grid %u,%u,%u block %u lds %zu args", n.c_str(), g.x, g.y, g.z, b.x, shmem);
    int cnt; const int* sz = sizes(n, cnt);
    for (int i = 0; i < cnt; ++i) {
        fprintf(out, " ");
        const unsigned char* p = (const unsigned char*)args[i];
        if (sz[i] == 4) fprintf(out, "%d", *(const int*)p);
        else if (sz[i] == 8) fprintf(out, "%llx", *(const unsigned long long*)p);
        else { uint32_t h = 2166136261u; for (int k = 0; k < sz[i]; ++k) h = (h ^ p[k]) * 16777619u; fprintf(out, "#%08x", h); }
    }
    fprintf(out, "\n");
    return hipSuccess;
}
static dim3 cfg_g, cfg_b; static size_t cfg_s; static hipStream_t cfg_st;
extern "C" hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t s, hipStream_t st) { cfg_g = g; cfg_b = b; cfg_s = s; cfg_st = st; return hipSuccess; }
extern "C" hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* s, hipStream_t* st) { *g = cfg_g; *b = cfg_b; *s = cfg_s; *st = cfg_st; return hipSuccess; }
extern "C" hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
extern "C" hipError_t hipGetLastError() { return hipSuccess; }
extern "C" hipError_t hipPeekAtLastError() { return hipSuccess; }
extern "C" hipError_t hipMemsetD32Async(hipDeviceptr_t d, int v, size_t n, hipStream_t) { fprintf(out, "  memsetD32 %p %d %zu\n", d, v, n); return hipSuccess; }

static void* P(uintptr_t v) { return (void*)v; }
static const size_t BIG = (size_t)1 << 40;
static void igemm_all(int B, int D, int H, int W, int cin, int cout, int k, int s, int pad) {
    const int Do = (D + 2 * pad - k) / s + 1, Ho = (H + 2 * pad - k) / s + 1, Wo = (W + 2 * pad - k) / s + 1;
    for (int tr = 0; tr < (s == 1 ? 2 : 1); ++tr) for (int add = 0; add < 2; ++add) for (int ws = 0; ws < 2; ++ws) for (int of = 0; of < 2; ++of) {
        fprintf(out, "igemm_ws B%d %dx%dx%d %d->%d k%d s%d tr%d add%d ws%d of%d\n", B, D, H, W, cin, cout, k, s, tr, add, ws, of);
        int rc = dreg_conv3d_igemm_ws(P(0x1000), P(0x2000), P(0x3000), add ? (const float*)P(0x4000) : nullptr, add ? P(0x5000) : nullptr, B, D, H, W, cin, Do, Ho, Wo, cout, k, s, pad, tr, add, Do, Ho, Wo, 1,
                                      0, of, ws ? P(0x6000) : nullptr, ws ? BIG : 0, nullptr);
        fprintf(out, "  rc %d\n", rc);
    }
    int rpc = -1, nsp = -1; size_t slc = 0;
    fprintf(out, "bnstats/defer/occ/f32/rows\n");
    int rc = dreg_conv3d_igemm_bnstats(P(0x1000), P(0x2000), P(0x3000), nullptr, nullptr, B, D, H, W, cin, Do, Ho, Wo, cout, k, s, pad, 0, 0, 0, 0, 0, P(0x6000), BIG, (float*)P(0x7000), &rpc, nullptr);
    fprintf(out, "  rc %d rpc %d\n", rc, rpc);
    rc = dreg_conv3d_igemm_defer(P(0x1000), P(0x2000), P(0x3000), nullptr, nullptr, B, D, H, W, cin, Do, Ho, Wo, cout, k, s, pad, 0, 0, 0, 0, 0, 0, P(0x6000), BIG, (const uint8_t*)P(0x8000), &nsp, &slc, nullptr);
    fprintf(out, "  rc %d nsplit %d slice %zu\n", rc, nsp, slc);
    rc = dreg_conv3d_igemm_occ(P(0x1000), P(0x2000), P(0x3000), nullptr, nullptr, B, D, H, W, cin, Do, Ho, Wo, cout, k, s, pad, 0, 0, 0, 0, 0, 0, 0, 0, nullptr, 0, (const uint8_t*)P(0x8000), nullptr);
    fprintf(out, "  rc %d\n", rc);
    rc = dreg_conv3d_igemm_ws(P(0x1000), P(0x2000), P(0x3000), nullptr, nullptr, B, D, H, W, cin, Do, Ho, Wo, cout, k, s, pad, 0, 1, 0, 0, 0, 0, 1, 0, nullptr, 0, nullptr);
    fprintf(out, "  rc %d\n", rc);
    const int M = B * Do * Ho * Wo;
    for (int n : {M / 3 + 1, 16384, 70000}) if (n <= M) {
        rc = dreg_conv3d_igemm_rows(P(0x1000), P(0x2000), P(0x3000), nullptr, nullptr, (const int*)P(0x9000), n, B, D, H, W, cin, Do, Ho, Wo, cout, k, s, pad, 0, 0, 0, 0, 0, 0, 0, nullptr);
        fprintf(out, "  rows %d rc %d\n", n, rc);
    }
}
static void wgrad_all(int B, int D, int H, int W, int cin, int cout, int k) {
    const int pad = k / 2;
    fprintf(out, "wgrad B%d %dx%dx%d %d->%d k%d\n", B, D, H, W, cin, cout, k);
    for (int dt = 0; dt < 2; ++dt) for (int tr = 0; tr < 2 - dt; ++tr) for (int occ = 0; occ < 2; ++occ) {
        int rc = dreg_conv3d_wgrad_occ(P(0x1000), P(0x2000), (float*)P(0x3000), P(0x4000), BIG, B, D, H, W, cin, cin, D, H, W, cout, k, 1, pad, 1, dt, tr, occ ? (const uint8_t*)P(0x8000) : nullptr, nullptr);
        fprintf(out, "  dt%d tr%d occ%d rc %d\n", dt, tr, occ, rc);
    }
    const long M = (long)B * D * H * W;
    for (int n : {1000, 16383, 16384, 28000, 65535, 65536, 90000, 200000}) if (n <= M) {
        int rc = dreg_conv3d_wgrad_rows(P(0x1000), P(0x2000), (float*)P(0x3000), P(0x4000), BIG, (const int*)P(0x9000), n, B, D, H, W, cin, cin, D, H, W, cout, k, 1, pad, 0, nullptr);
        fprintf(out, "  rows %d rc %d\n", n, rc);
        rc = dreg_conv3d_wgrad_partials(P(0x1000), P(0x2000), P(0x4000), BIG, (const int*)P(0x9000), n, B, D, H, W, cin, cin, D, H, W, cout, k, 1, pad, nullptr, nullptr);
        fprintf(out, "  partials rows %d rc %d\n", n, rc);
    }
    for (int v : {128128, 128064, 64128, 64064, 256256}) { int rc = dreg_wgrad_group_launch(P(0xa000), 3, v, 77, nullptr); fprintf(out, "  group %d rc %d\n", v, rc); }
}
static void sweep() {
    for (int B : {1, 2, 8}) for (int D : {1, 4, 8, 16, 32, 64}) for (int cin : {64, 128, 256, 512, 1024}) for (int cout : {64, 128, 256, 512}) for (int k : {1, 3}) {
        igemm_all(B, D, D, D, cin, cout, k, 1, k / 2);
        wgrad_all(B, D, D, D, cin, cout, k);
    }
    igemm_all(1, 64, 32, 32, 64, 256, 1, 1, 0); wgrad_all(1, 64, 32, 32, 256, 256, 1); wgrad_all(1, 64, 32, 32, 64, 256, 3); wgrad_all(1, 64, 64, 16, 64, 256, 3); wgrad_all(1, 8, 8, 64, 64, 64, 3);
    igemm_all(8, 128, 128, 128, 8, 64, 5, 2, 2); igemm_all(1, 16, 16, 16, 8, 64, 5, 2, 2); igemm_all(8, 32, 32, 32, 64, 128, 3, 2, 1);
    wgrad_all(9856, 1, 1, 1, 256, 256, 1); wgrad_all(8, 64, 64, 64, 256, 256, 5); wgrad_all(8, 32, 32, 32, 128, 128, 5);
    for (int k : {1, 3}) for (int acc = 0; acc < 2; ++acc) for (int D : {16, 32, 64}) for (int cin : {64, 128}) {
        const int pad = k / 2, Do = (D + 2 * pad - k) / 2 + 1;
        fprintf(out, "dgrad_s2 k%d acc%d D%d cin%d\n", k, acc, D, cin);
        int rc = (acc ? dreg_conv3d_dgrad_s2_acc : dreg_conv3d_dgrad_s2)(P(0x1000), P(0x2000), P(0x3000), 8, D, D, D, cin, Do, Do, Do, 2 * cin, k, pad, nullptr);
        fprintf(out, "  rc %d\n", rc);
    }
}
int main(int argc, char** argv) {
    if (argc > 1) out = fopen(argv[1], "w");
    fprintf(out, "== defaults\n"); sweep();
#ifdef PROBE
    struct K { const char* n; void (*f)(int); int v, d; };
    const K ks[] = {{"glds", dreg_conv_set_glds, 0, 1}, {"glds", dreg_conv_set_glds, 2, 1}, {"glds", dreg_conv_set_glds, 3, 1}, {"glds", dreg_conv_set_glds, 4, 1}, {"glds", dreg_conv_set_glds, 5, 1},
        {"wgrad_big", dreg_conv_set_wgrad_big, 0, 3}, {"wgrad_big", dreg_conv_set_wgrad_big, 1, 3}, {"wgrad_big", dreg_conv_set_wgrad_big, 11, 3}, {"wgrad_big", dreg_conv_set_wgrad_big, 12, 3}, {"wgrad_big", dreg_conv_set_wgrad_big, 13, 3},
        {"wgrad_ring", dreg_conv_set_wgrad_ring, 0, 3}, {"wgrad_ring", dreg_conv_set_wgrad_ring, 1, 3}, {"wgrad_ring", dreg_conv_set_wgrad_ring, 2, 3}, {"wgrad_ring", dreg_conv_set_wgrad_ring, 4, 3}, {"wgrad_ring", dreg_conv_set_wgrad_ring, 5, 3},
        {"wgrad_ring", dreg_conv_set_wgrad_ring, 6, 3}, {"wgrad_ring", dreg_conv_set_wgrad_ring, 7, 3}, {"wgrad_ring", dreg_conv_set_wgrad_ring, 8, 3}, {"wgrad_pipe", dreg_conv_set_wgrad_pipe, 1, 0},
        {"rows_fast", dreg_conv_set_wgrad_rows_fast, 0, 1}, {"row_splits", dreg_conv_set_row_splits, 0, 1}, {"narrow_small", dreg_conv_set_narrow_small, 0, 2}, {"narrow_small", dreg_conv_set_narrow_small, 1, 2},
        {"igemm_probe", dreg_conv_igemm_probe, 1, 0}, {"igemm_ap", dreg_conv_set_igemm_ap, 0, 256}, {"igemm_ap256", dreg_conv_set_igemm_ap256, 0, 1}, {"rmw_cin", dreg_conv_set_pointwise_rmw_cin, 0, 128},
        {"glds_stages", dreg_conv_set_glds_stages, 3, 0}, {"glds_stages", dreg_conv_set_glds_stages, 4, 0}, {"bn_stats", dreg_conv_set_bn_stats_epilogue, 0, 1}, {"wgrad_splits", dreg_conv_set_wgrad_splits, 7, 0}};
    for (const K& k : ks) { fprintf(out, "== %s=%d\n", k.n, k.v); k.f(k.v); sweep(); k.f(k.d); }
    fprintf(out, "== ring0+pipe1\n"); dreg_conv_set_wgrad_ring(0); dreg_conv_set_wgrad_pipe(1); sweep(); dreg_conv_set_wgrad_ring(3); dreg_conv_set_wgrad_pipe(0);
#endif
    return 0;
}
