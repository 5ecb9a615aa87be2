// libnsh_hip.so: rational_resampler_ccf, resample by I/D (GNU Radio semantics: zero-stuff by I,
// filter with L real taps, keep every D-th sample).
//
//   y[n] = sum_{k<L} h[k] u[nD - k],   u[jI] = x[j], u = 0 elsewhere
//        = sum_{q<Q} h[phi + qI] x[j0 - q],   phi = (nD) mod I,  j0 = floor(nD / I),  Q = ceil(L / I)
//
// 1 <= I <= 64, 1 <= D <= 64, 1 <= L <= 1024, I and D used as given (not reduced by their gcd).
// Larger ratios (160/147 and the like) and rates that are no ratio are k_arb's (nsh_arb.hip).
// A call processes n_units units of D inputs and I outputs each, so every call starts at phase 0
// and the only state is the history: the Q-1 raw samples before in[0].
//
//   k_resamp<R,P>  one launch per call. A 256-thread workgroup makes U = G R units: G groups of R
//                consecutive units, G = min(256 / I, 8192 / (R D)) (at least 1), so a tile is
//                about 256 R outputs when I >= D and at most 8192 inputs when D > I.
//     stage      The tile's U D + Q-1 samples, each read from HBM once per workgroup with 8-byte
//                non-temporal loads (ring pointers are only 8-byte aligned), 8 pairs per lane in
//                flight as in k_fir_xlat. The stream's first and last tiles read through virt()
//                (history, zeros). The taps go to LDS in their own order, hs[k] = h[k]: tap q of
//                phase phi is hs[phi + q I].
//     FIR        Lane w = g I + r (r fastest) keeps output-in-unit index r of R units: g + t G in
//                k_resamp<8,1> (D <= I), the consecutive g R + t in the others. They share
//                phi = (r D) mod I and their windows lie a multiple of D apart, so the lane reads
//                a tap once per R outputs. q ascending, one FMA per component and step: the
//                order is fixed per output, whatever the tile and the call it falls into. Taps
//                k = phi + q I >= L (the padding up to Q I) are skipped, never multiplied (0 x NaN
//                would poison an output whose L-tap sum does not hold the sample): only the last
//                q can hold one, and it takes a per-lane test.
//     banks      A ds_read_b64 serves lanes 0-31 and 32-63 separately, bank pair = entry mod 32.
//                k_resamp<8,1> (D <= I): the lanes of a group read samples
//                c + g D + floor(r D / I), which never decrease along w and rise by at most one
//                per lane: at most 32 consecutive samples (equal ones are a broadcast),
//                conflict-free with the image packed, sample s at entry s, and the address is
//                linear in q (the reads of an unrolled step differ by immediate offsets).
//                The others (D > I): the same mapping would put two to three entries on a bank
//                pair (measured slower at (2, 3) and (4, 5) than the padded image),
//                and lanes R D apart share bank pairs for most D, as in k_fir_xlat, whose padding
//                they take: sample s at entry s + (s >> a); the plan picks the a in
//                {31 (none), 6, ..., 1} with the smallest worst-case multiplicity over the lane
//                groups and every window offset c (ties: the larger a, the smaller image). With
//                I = 1 (one stride) that is conflict-free; with the second stride floor(r D / I)
//                one shift cannot serve both and up to three entries share a bank pair. k_pfb's
//                free row needs rows of a fixed pitch, which these windows do not have.
//                tests/test_resamp_layout.py recomputes all of this and asserts it.
//                Tap reads (ds_read_b32, bank = k mod 32): the phases of a lane group are distinct
//                or equal below I = 32 and at most two to a bank above; one per R sample reads.
//     store      Through LDS: after a barrier the lanes write their outputs over the sample image
//                at their place in the tile, unit I + r, and the workgroup reads the tile back
//                linearly: 16-byte non-temporal stores when out is 16-byte aligned and the tile
//                has an even number of outputs, the 8-byte path otherwise.
//   Instantiations by D / I: <8,1> D <= I (packed image), then padded <8,0> D <= 2 I, <4,0> D <= 4 I,
//   <2,0> D <= 8 I, <1,0> above.
//   Accuracy: fp32 throughout. Non-finite samples propagate by IEEE arithmetic: output n is
//   non-finite exactly when one of its L-tap products holds the sample.
#include "nsh_common.hpp"

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

namespace {

constexpr int kBlock = 256;
constexpr int kStage = 8;        // sample pairs a lane loads before it stores the first
constexpr int kMaxTileIn = 8192; // inputs of a tile when D > I

using nsh::ld_nt;
using nsh::nf2;
using nsh::nf4;
using nsh::virt;

template <int R, bool kLinear>
__global__ __launch_bounds__(kBlock) void k_resamp(const float2* __restrict__ in,
                                                   const float2* __restrict__ hist_in,
                                                   float2* __restrict__ hist_out,
                                                   float2* __restrict__ out,
                                                   const float* __restrict__ taps, // h[k], Q I floats (zero padded)
                                                   int L,
                                                   int I,
                                                   int D,
                                                   int Q,
                                                   int G,     // groups of R units per workgroup
                                                   int a,     // !kLinear: LDS entry of sample s is s + (s >> a)
                                                   int hs_at, // first float2 entry of the taps in LDS
                                                   int64_t n_units,
                                                   int vec) // 16-byte stores
{
    extern __shared__ __attribute__((aligned(16))) float2 xs[];
    float* hs = reinterpret_cast<float*>(xs + hs_at);

    const auto entry = [a](int s) { return kLinear ? s : s + (s >> a); };
    const int tid = threadIdx.x;
    const int U = G * R;
    const int H = Q - 1;
    const int64_t n_in = n_units * D;
    const int64_t u0 = (int64_t)blockIdx.x * U; // the tile's first unit
    const int64_t g0 = u0 * D - H;              // stream sample (of this call) at window position 0
    const int count = U * D + H;

    auto stage = [&](auto load) {
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
                if (i < count) {
                    xs[entry(i)] = x0[u];
                    if (i + 1 < count) xs[entry(i + 1)] = x1[u];
                }
            }
        }
    };
    if (g0 >= 0 && g0 + count <= n_in)
        stage([&](int i) { return ld_nt(in + g0 + i); });
    else
        stage([&](int i) { return virt(in, hist_in, g0 + i, n_in, Q); });
    for (int i = tid; i < Q * I; i += kBlock) hs[i] = taps[i];
    if (blockIdx.x == 0) { // history for the next call: the Q-1 raw samples before in[n_in]
        for (int j = tid; j < H; j += kBlock) hist_out[j] = virt(in, hist_in, n_in - H + j, n_in, Q);
    }
    __syncthreads();

    const bool active = tid < G * I;
    const int g = active ? tid / I : 0;
    const int r = active ? tid - g * I : 0;
    const int rd = r * D;
    const int base = rd / I;       // floor(r D / I): the unit's newest sample for this output
    const int phi = rd - base * I; // (r D) mod I
    const int qall = L / I;        // taps every phase has: q < qall
    float2 acc[R];
#pragma unroll
    for (int t = 0; t < R; ++t) acc[t] = make_float2(0.f, 0.f);
    const int ug = kLinear ? g : g * R; // the lane's units: ug + t ut
    const int ut = kLinear ? G : 1;
    if (active) {
        const int s0 = H + ug * D + base; // window position of x[j0] of the lane's first unit
#pragma unroll 4
        for (int q = 0; q < qall; ++q) {
            const float h = hs[phi + q * I];
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const float2 x = xs[entry(s0 + t * ut * D - q)];
                acc[t].x = __builtin_fmaf(h, x.x, acc[t].x);
                acc[t].y = __builtin_fmaf(h, x.y, acc[t].y);
            }
        }
        if (qall < Q && phi + qall * I < L) { // the last, partial row of taps
            const float h = hs[phi + qall * I];
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const float2 x = xs[entry(s0 + t * ut * D - qall)];
                acc[t].x = __builtin_fmaf(h, x.x, acc[t].x);
                acc[t].y = __builtin_fmaf(h, x.y, acc[t].y);
            }
        }
    }
    __syncthreads(); // every lane is done with the samples: the tile's outputs take their place
    if (active) {
#pragma unroll
        for (int t = 0; t < R; ++t) xs[(ug + t * ut) * I + r] = acc[t];
    }
    __syncthreads();

    const int64_t n_out = n_units * I;
    const int64_t o0 = u0 * I; // the tile's first output
    const int tile_out = U * I;
    if (vec) { // tile_out and o0 are even
        for (int e = 2 * tid; e < tile_out; e += 2 * kBlock) {
            if (o0 + e + 1 < n_out) {
                const nf4 v = *reinterpret_cast<const nf4*>(xs + e);
                __builtin_nontemporal_store(v, reinterpret_cast<nf4*>(out + o0 + e));
            } else if (o0 + e < n_out) {
                const nf2 v = *reinterpret_cast<const nf2*>(xs + e);
                __builtin_nontemporal_store(v, reinterpret_cast<nf2*>(out + o0 + e));
            }
        }
    } else {
        for (int e = tid; e < tile_out; e += kBlock) {
            if (o0 + e < n_out) {
                const nf2 v = *reinterpret_cast<const nf2*>(xs + e);
                __builtin_nontemporal_store(v, reinterpret_cast<nf2*>(out + o0 + e));
            }
        }
    }
}

struct resamp_plan {
    int dev = 0;
    int L = 0, I = 0, D = 0, Q = 0;
    int R = 0, G = 0, U = 0; // units per workgroup U = G R
    bool linear = false; // the packed image, a lane's units G apart
    int a = 0, hs_at = 0;
    size_t lds = 0;
    float* taps_dev = nullptr;
    // the instantiation, chosen once at plan creation (pick): the kernel and its launcher
    const void* fn = nullptr;
    void (*launch)(const resamp_plan*, const float2*, const float2*, float2*, float2*, int64_t, int, unsigned,
                   hipStream_t) = nullptr;
    std::string kernel;

    resamp_plan() = default;
    resamp_plan(const resamp_plan&) = delete;
    resamp_plan& operator=(const resamp_plan&) = delete;
    ~resamp_plan() { nsh::dev_free(taps_dev); }
};

template <int R, bool kLinear>
void launch_resamp(const resamp_plan* p, const float2* in, const float2* hin, float2* hout, float2* out, int64_t n_units,
                   int vec, unsigned grid, hipStream_t s)
{
    nsh::launch((k_resamp<R, kLinear>), dim3(grid), dim3(kBlock), (uint32_t)p->lds, s, in, hin, hout, out, (const float*)p->taps_dev,
                p->L, p->I, p->D, p->Q, p->G, p->a, p->hs_at, n_units, vec);
}

template <int R, bool kLinear>
void pick(resamp_plan* p)
{
    p->R = R;
    p->linear = kLinear;
    p->fn = (const void*)k_resamp<R, kLinear>;
    p->launch = launch_resamp<R, kLinear>;
}

// Worst number of different entries on one bank pair among the 32 lanes of a ds_read_b64 group,
// over the lane groups of the workgroup and every window offset, with sample s at s + (s >> a).
int worst_multiplicity(int I, int D, int R, int G, int a)
{
    int worst = 1;
    for (int c = 0; c < 64; ++c)
        for (int l0 = 0; l0 < kBlock && l0 < G * I; l0 += 32) {
            int entry[32][32], n[32] = {};
            for (int w = l0; w < l0 + 32 && w < G * I; ++w) {
                const int s = c + (w / I) * R * D + (w % I) * D / I, e = s + (s >> a), b = e & 31;
                bool seen = false;
                for (int i = 0; i < n[b]; ++i) seen = seen || entry[b][i] == e;
                if (!seen) entry[b][n[b]++] = e;
            }
            for (int b = 0; b < 32; ++b) worst = std::max(worst, n[b]);
        }
    return worst;
}

} // namespace

extern "C" {

int nsh_resamp_plan_create(int dev, const float* taps_host, int ntaps, int interp, int decim, void** plan)
{
    if (!taps_host || !plan) return nsh::fail_msg("nsh_resamp_plan_create: null pointer");
    if (ntaps < 1 || ntaps > 1024) return nsh::fail_msg("nsh_resamp_plan_create: ntaps must be in [1, 1024]");
    if (interp < 1 || interp > 64) return nsh::fail_msg("nsh_resamp_plan_create: interpolation must be in [1, 64]");
    if (decim < 1 || decim > 64) return nsh::fail_msg("nsh_resamp_plan_create: decimation must be in [1, 64]");
    NSH_CK(hipSetDevice(dev));
    auto p = std::make_unique<resamp_plan>();
    p->dev = dev;
    p->L = ntaps;
    p->I = interp;
    p->D = decim;
    p->Q = (ntaps + interp - 1) / interp;
    if (decim <= interp)
        pick<8, true>(p.get());
    else if (decim <= 2 * interp)
        pick<8, false>(p.get());
    else if (decim <= 4 * interp)
        pick<4, false>(p.get());
    else if (decim <= 8 * interp)
        pick<2, false>(p.get());
    else
        pick<1, false>(p.get());
    p->G = std::max(1, std::min(kBlock / interp, kMaxTileIn / (p->R * decim)));
    p->U = p->G * p->R;
    p->kernel = "k_resamp<" + std::to_string(p->R) + (p->linear ? ",1>" : ",0>");
    p->a = 31; // no padding: k_resamp<8,1>'s packed image
    if (!p->linear) {
        int best = 1 << 30;
        for (int a : { 31, 6, 5, 4, 3, 2, 1 }) {
            const int m = worst_multiplicity(interp, decim, p->R, p->G, a);
            if (m < best) best = m, p->a = a;
        }
    }
    // the sample image (the tile's outputs take its place later), then the taps, 16-byte aligned
    const int wn = p->U * decim + p->Q - 1;
    p->hs_at = (std::max(wn + (wn >> p->a) + 1, p->U * interp) + 1) / 2 * 2;
    p->lds = (size_t)p->hs_at * sizeof(float2) + (size_t)p->Q * interp * sizeof(float);
    // at most 112 KiB (8192 inputs, L = 1024, a = 1), within the CU's 160 KiB
    hipError_t e = hipFuncSetAttribute(p->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->lds);
    std::vector<float> host((size_t)p->Q * interp, 0.f);
    std::copy(taps_host, taps_host + ntaps, host.begin());
    if (e == hipSuccess) e = hipMalloc(&p->taps_dev, host.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(p->taps_dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) return nsh::fail(e, "nsh_resamp_plan_create");
    *plan = p.release();
    return 0;
}

int nsh_resamp_plan_destroy(void* plan)
{
    delete static_cast<resamp_plan*>(plan);
    return 0;
}

int nsh_resamp_tile(void* plan) { return plan ? static_cast<resamp_plan*>(plan)->U : 0; }
const char* nsh_resamp_kernel(void* plan) { return plan ? static_cast<resamp_plan*>(plan)->kernel.c_str() : ""; }
int nsh_resamp_history(void* plan) { return plan ? static_cast<resamp_plan*>(plan)->Q - 1 : 0; }

int nsh_resamp_ccf(void* plan, const float* in, const float* hist_in, float* hist_out, float* out, int64_t n_units,
                   void* stream)
{
    nsh::launch_events_guard timing_guard; // the armed event pair never outlives this call
    auto* p = static_cast<resamp_plan*>(plan);
    // what needs no plan comes first, as in check_stream_call
    if (hist_in && hist_in == hist_out) return nsh::fail_msg("nsh_resamp_ccf: hist_out must not alias hist_in");
    if (n_units > 0 && (!in || !out)) return nsh::fail_msg("nsh_resamp_ccf: null input or output");
    if (!p) return nsh::fail_msg("nsh_resamp_ccf: null plan");
    if (n_units <= 0) return 0;
    if (!hist_out && p->Q > 1) return nsh::fail_msg("nsh_resamp_ccf: hist_out is required (ceil(ntaps / interp) - 1 samples)");
    const int64_t grid = (n_units + p->U - 1) / p->U;
    if (grid > 0x7fffffff || n_units > INT64_MAX / 128) return nsh::fail_msg("nsh_resamp_ccf: too many units for one call");
    const int vec = (uintptr_t)out % 16 == 0 && (p->U * p->I) % 2 == 0 ? 1 : 0;
    p->launch(p, (const float2*)in, (const float2*)hist_in, (float2*)hist_out, (float2*)out, n_units, vec, (unsigned)grid,
              nsh::S(stream));
    NSH_CK_LAUNCH("nsh_resamp_ccf");
    return 0;
}

} // extern "C"
