// Probe for "request the first bytes before any kernarg wait" (DESIGN.md 6g''): what does the scalar round trip for the kernel
// arguments cost a small dependent kernel whose kernarg lines are cold, and does the firmware place leading plain arguments in
// user SGPRs when the code object asks for it (-mllvm -amdgpu-kernarg-preload-count=N)?
// A captured graph of one 64 MB once-read stream (it pushes the previous replay's kernarg lines out of L2) followed by CHAIN
// dependent small launches on one stream; every launch loads 16 B per lane through a pointer argument and stores one float per lane.
// The per-launch figure is (replay with the chain - replay of the stream alone) / CHAIN, median of REPS replays.
//   struct   arguments in a by-value struct (never preloaded): s_load, wait, global_load
//   plain    the same four values as leading plain arguments: with the flag the global_load needs no s_load at all
//   empty    a kernel without arguments or body: the launch floor
// Build it twice and run both; the binaries differ in the `plain` row only:
//   hipcc --offload-arch=gfx950 -O3 tools/probe/kernarg_preload.hip -o tools/probe/kernarg_preload_off_bin
//   hipcc --offload-arch=gfx950 -O3 -mllvm -amdgpu-kernarg-preload-count=16 -DKPL_FLAG tools/probe/kernarg_preload.hip -o tools/probe/kernarg_preload_on_bin
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <algorithm>
#include <vector>

#define CHAIN 400
#define REPS 21
#define BLOCKS 64
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

struct P { const float4* a; float* out; int stride; int salt; };

__global__ __launch_bounds__(256) void k_struct(P p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const float4 v = p.a[(size_t)i * p.stride];
    p.out[i] = (v.x + v.y) + (v.z + v.w) + (float)p.salt;
}
__global__ __launch_bounds__(256) void k_plain(const float4* a, float* out, int stride, int salt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const float4 v = a[(size_t)i * stride];
    out[i] = (v.x + v.y) + (v.z + v.w) + (float)salt;
}
__global__ void k_empty() {}
typedef __attribute__((ext_vector_type(4))) unsigned int u4;
__global__ __launch_bounds__(256) void k_stream(const u4* __restrict__ p, size_t n16, unsigned* sink) {
    u4 acc = {0, 0, 0, 0};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) {
        acc ^= __builtin_nontemporal_load(p + i);
    }
    if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x12345678u) sink[0] = 1;
}

// mode 0: stream only, 1: + struct chain, 2: + plain chain, 3: + empty chain
static int capture(int mode, hipStream_t st, const u4* big, size_t n16, unsigned* sink, const float4* a, float* out, hipGraphExec_t* exec) {
    hipGraph_t g;
    CK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    hipLaunchKernelGGL(k_stream, dim3(2048), dim3(256), 0, st, big, n16, sink);
    for (int i = 0; i < (mode ? CHAIN : 0); ++i) {
        if (mode == 1) hipLaunchKernelGGL(k_struct, dim3(BLOCKS), dim3(256), 0, st, P{a, out, 1, i});
        else if (mode == 2) hipLaunchKernelGGL(k_plain, dim3(BLOCKS), dim3(256), 0, st, a, out, 1, i);
        else hipLaunchKernelGGL(k_empty, dim3(BLOCKS), dim3(256), 0, st);
    }
    CK(hipStreamEndCapture(st, &g));
    CK(hipGraphInstantiate(exec, g, nullptr, nullptr, 0));
    CK(hipGraphDestroy(g));
    return 0;
}

static int replay_us(hipGraphExec_t exec, hipStream_t st, double* med) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<double> t;
    for (int r = 0; r < REPS + 3; ++r) {
        CK(hipEventRecord(e0, st));
        CK(hipGraphLaunch(exec, st));
        CK(hipEventRecord(e1, st));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 3) t.push_back(ms * 1e3);
    }
    std::sort(t.begin(), t.end());
    *med = t[t.size() / 2];
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
    return 0;
}

int main() {
    const size_t big_bytes = (size_t)64 << 20, n16 = big_bytes / 16;
    const size_t n = (size_t)BLOCKS * 256;
    u4* big; unsigned* sink; float4* a; float* out;
    CK(hipMalloc(&big, big_bytes)); CK(hipMalloc(&sink, 4)); CK(hipMalloc(&a, n * sizeof(float4))); CK(hipMalloc(&out, n * sizeof(float)));
    CK(hipMemset(big, 1, big_bytes)); CK(hipMemset(sink, 0, 4)); CK(hipMemset(a, 0, n * sizeof(float4))); CK(hipMemset(out, 0, n * sizeof(float)));
    hipStream_t st;
    CK(hipStreamCreate(&st));
    const char* names[4] = {"stream only", "struct", "plain", "empty"};
    double us[4];
    for (int mode = 0; mode < 4; ++mode) {
        hipGraphExec_t exec;
        if (capture(mode, st, big, n16, sink, a, out, &exec)) return 1;
        if (replay_us(exec, st, &us[mode])) return 1;
        CK(hipGraphExecDestroy(exec));
    }
#ifdef KPL_FLAG
    const char* build = "kernarg-preload-count=16";
#else
    const char* build = "no preload flag";
#endif
    printf("# build: %s; %d dependent launches of %d x 256 threads behind a 64 MB once-read stream, median of %d replays\n", build, CHAIN, BLOCKS, REPS);
    printf("# %-12s %14s %14s\n", "arguments", "replay us", "us / launch");
    printf("  %-12s %14.1f %14s\n", names[0], us[0], "-");
    for (int mode = 1; mode < 4; ++mode) printf("  %-12s %14.1f %14.3f\n", names[mode], us[mode], (us[mode] - us[0]) / CHAIN);
    // the chain's result: out[i] = 0 + salt of the last launch
    float h;
    CK(hipMemcpy(&h, out, 4, hipMemcpyDeviceToHost));
    if (h != (float)(CHAIN - 1)) { printf("unexpected result %g\n", h); return 1; }
    return 0;
}
