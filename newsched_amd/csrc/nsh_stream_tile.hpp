// What the one-launch stream kernels share: k_fir_xlat (nsh_xlat.hip), k_pfb (nsh_pfb.hip), k_resamp
// (nsh_resamp.hip) and k_arb (nsh_arb.hip). A workgroup stages the window of its tile in LDS, each
// sample read from HBM once, filters from LDS, and workgroup 0 writes the history of the next call.
// Device pieces first (they take tid as a parameter: reading threadIdx.x again in a helper moves the
// callers' code), then the plans' common part and the entry points' argument checks. All four use
// fma2, the plan base and, but for nsh_arb_resamp_ccf, the checks; stage_window serves k_resamp and
// k_arb, store_history k_pfb, k_resamp and k_fft_xlat (nsh_fft_xlat_kernel.hpp), store_tile k_resamp and k_arb. A kernel that keeps a loop
// of its own says at the loop what the shared one cost it (assembly or time).
#pragma once
#include "nsh_common.hpp"

#include "nsh_stream_layout.hpp"

namespace nsh {

// Stages window positions [0, count): a lane takes two neighbouring samples, kStage pairs per pass,
// and every load of a pass is issued before the first sample is put (a pass of one pair per lane
// waits out the HBM latency 16 times per 8192-sample window). load(i) is sample i of
// the window: a workgroup whose window lies inside the input loads it directly, the stream's first
// and last ones through virt() (history, zeros); the kernel chooses. put(i, x0, x1) places samples
// i and i + 1 in the kernel's LDS image; i is even and below count, i + 1 may be count.
// A kernel calls this from one generic lambda of its own, stage(load), for both loaders: called at
// the two sites directly, the loop's addressing came out otherwise and k_resamp and k_arb measured
// 1 to 6 % slower on some legs (profiles/stream_refactor_ab.log).
template <int kBlock, int kStage, typename Load, typename Put>
__device__ __forceinline__ void stage_window(int count, int tid, Load load, Put put)
{
    for (int i0 = 2 * tid; i0 < count; i0 += 2 * kBlock * kStage) {
        float2 x0[kStage], x1[kStage];
#pragma unroll
        for (int u = 0; u < kStage; ++u) {
            const int i = i0 + 2 * kBlock * u;
            x0[u] = i < count ? load(i) : make_float2(0.f, 0.f);
            x1[u] = i + 1 < count ? load(i + 1) : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < kStage; ++u) {
            const int i = i0 + 2 * kBlock * u;
            if (i < count) put(i, x0[u], x1[u]);
        }
    }
}

// History for the next call, written by one workgroup: the L-1 raw samples before in[end], for a
// call that consumes its n_in = end inputs (k_arb, which may consume fewer, has the loop with both
// bounds: with end and n_in apart the compiler keeps a test here that it drops for one value).
template <int kBlock>
__device__ __forceinline__ void store_history(const float2* __restrict__ in, const float2* __restrict__ hist_in,
                                              float2* __restrict__ hist_out, int64_t end, int L, int tid)
{
    for (int j = tid; j < L - 1; j += kBlock) hist_out[j] = virt(in, hist_in, end - (L - 1) + j, end, L);
}

// The tile's outputs, which lie in LDS in their order from xs[0], to out[o0 ..]: the workgroup
// reads them back linearly, 16-byte non-temporal stores when vec (out is 16-byte aligned, tile and
// so o0 are even: store_vec16), the 8-byte path otherwise. Nothing at or past n_out is stored.
template <int kBlock>
__device__ __forceinline__ void store_tile(const float2* xs, float2* __restrict__ out, int64_t o0, int tile, int64_t n_out,
                                           int vec, int tid)
{
    if (vec) {
        for (int e = 2 * tid; e < tile; e += 2 * kBlock) {
            if (o0 + e + 1 < n_out) {
                const nf4 v = *reinterpret_cast<const nf4*>(xs + e);
                __builtin_nontemporal_store(v, reinterpret_cast<nf4*>(out + o0 + e));
            } else if (o0 + e < n_out) {
                const nf2 v = *reinterpret_cast<const nf2*>(xs + e);
                __builtin_nontemporal_store(v, reinterpret_cast<nf2*>(out + o0 + e));
            }
        }
    } else {
        for (int e = tid; e < tile; e += kBlock) {
            if (o0 + e < n_out) {
                const nf2 v = *reinterpret_cast<const nf2*>(xs + e);
                __builtin_nontemporal_store(v, reinterpret_cast<nf2*>(out + o0 + e));
            }
        }
    }
}

// acc += h x, real times complex: one FMA per component (the build has -ffp-contract=off)
__device__ __forceinline__ void fma2(float2& acc, float h, float2 x)
{
    acc.x = __builtin_fmaf(h, x.x, acc.x);
    acc.y = __builtin_fmaf(h, x.y, acc.y);
}

// 16-byte stores of a tile: out is 16-byte aligned and every tile starts at an even output
inline int store_vec16(const void* out, int tile_out) { return (uintptr_t)out % 16 == 0 && tile_out % 2 == 0 ? 1 : 0; }

// The common part of a stream kernel's plan: the instantiation chosen at plan creation, its dynamic
// LDS and the one device buffer that holds the plan's constants (taps, twiddles).
struct stream_plan {
    int dev = 0;
    int tile = 0; // what a workgroup makes: outputs (units in k_resamp, time steps in k_pfb)
    int hist = 0; // samples of the carried history
    size_t lds = 0;
    const void* fn = nullptr;
    std::string kernel;
    void* buf = nullptr;

    stream_plan() = default;
    stream_plan(const stream_plan&) = delete;
    stream_plan& operator=(const stream_plan&) = delete;
    ~stream_plan() { dev_free(buf); }

    // Sets fn's dynamic-LDS limit and copies the constants to the device. The limit is set per plan,
    // not once per kernel (set_lds_attr): two live plans of one instantiation can differ in lds.
    int upload(const void* host, size_t bytes, const char* what)
    {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess) e = hipMalloc(&buf, bytes);
        if (e == hipSuccess) e = hipMemcpy(buf, host, bytes, hipMemcpyHostToDevice);
        return e == hipSuccess ? 0 : fail(e, what);
    }
};

// Argument checks of the stream entry points with one count (nsh_fir_xlat_ccf,
// nsh_pfb_channelizer_ccf, nsh_resamp_ccf), in their documented order; what needs no plan comes
// first, so that every refusal can be checked without a device. n counts items ("outputs",
// "units"), p->tile of them per workgroup; hist_len is the refusal's wording of p->hist. Returns the
// refusal's code, or 0 with *grid = the workgroups to launch (0: nothing to do).
inline int check_stream_call(const char* name, const stream_plan* p, const float* in, const float* hist_in,
                             const float* hist_out, const float* out, int64_t n, int64_t n_max, const char* hist_len,
                             const char* items, unsigned* grid)
{
    const auto refuse = [name](const std::string& what) { return fail_msg((name + what).c_str()); };
    *grid = 0;
    if (hist_in && hist_in == hist_out) return refuse(": hist_out must not alias hist_in");
    if (n > 0 && (!in || !out)) return refuse(": null input or output");
    if (!p) return refuse(": null plan");
    if (n <= 0) return 0;
    if (!hist_out && p->hist > 0) return refuse(std::string(": hist_out is required (") + hist_len + " samples)");
    const int64_t g = (n + p->tile - 1) / p->tile;
    if (g > 0x7fffffff || n > n_max) return refuse(std::string(": too many ") + items + " for one call");
    *grid = (unsigned)g;
    return 0;
}

} // namespace nsh
