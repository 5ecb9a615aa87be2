// libnsh_hip.so: rotator_cc and freq_xlating_fir_filter_ccf (tune, low-pass, decimate).
//
// Phase. A frequency is a 64-bit fixed-point phase increment in turns per sample,
// inc = round(frac(t) 2^64) mod 2^64, and the phase of absolute stream sample n is (n inc) mod 2^64
// turns in plain uint64 wrap-around arithmetic: it does not depend on how the stream is cut into
// calls and does not degrade with the stream position (a float phase accumulator leaves the 1e-5
// tolerance within seconds of stream). The phasor of a sample takes the top 32 bits of its phase
// as a signed number of half-turns (2^-24 half-turns of rounding, 1e-7 rad) through sincospif; the
// second sample of a 16-byte pair is the first one's phasor times the step phasor
// exp(j 2 pi inc / 2^64), computed in double on the host.
//
//   k_rotate        y[i] = x[i] exp(+j 2 pi phase(first_index + i)), 16 B per sample, ONE launch
//                   per call whatever n and the pointer alignment: ring pointers are only 8-byte
//                   aligned, so a misaligned head sample and an odd tail sample are rotated by two
//                   lanes of workgroup 0 inside the same launch; when in and out sit differently
//                   in their 16-byte slots every sample takes the 8-byte path. In place is allowed
//                   (every sample is read and written by the same lane, loads first).
//
//   k_fir_xlat<R,S> y[m] = sum_{k<L} h[k] (x[mD-k] exp(j 2 pi phase(first_index + mD - k))),
//                   D and L runtime values (1 <= D <= 64, 1 <= L <= 1024). A 256-thread workgroup
//                   stages the window of its T = 256 R / S outputs, (T-1) D + L samples, in LDS:
//                   one HBM read per sample plus the L-1 halo, rotated once at staging. Then the
//                   fp32 direct form with real taps: a lane keeps R consecutive outputs and walks
//                   the samples of its span in blocks of 8 (ds_read_b64); sample j of the span
//                   meets output r at reversed tap q = j - r D, which is wave-uniform, so the taps
//                   are scalar loads as in k_fir_direct. For large D the taps are split over S
//                   waves (part = wave mod S, uniform per wave) whose partial sums meet in LDS and
//                   are added in part order. Taps outside [0, L) are skipped, never multiplied
//                   (0 x inf would put a NaN where the L-tap sum has none).
//                   LDS image: sample s at entry s + (s >> a), 2^a the largest power of two in
//                   R D. A lane's span starts at s = g R D, so its entry stride is R D + (R D >> a),
//                   odd: the 32 lanes of a ds_read_b64 group fall on 32 different bank pairs.
//                   Instantiations by decimation, T D <= 8192 samples (two workgroups per CU on
//                   160 KiB when 2^a >= 8): D <= 4 <8,1>, <= 8 <4,1>, <= 16 <4,2>, <= 32 <4,4>,
//                   <= 64 <2,4>.
#include "nsh_phase.hpp"
#include "nsh_stream_tile.hpp"

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

namespace {

constexpr int kBlock = nsh::kStreamBlock;
constexpr int kUnroll = 4;
constexpr int kStage = 8; // sample pairs a lane loads before it rotates the first (k_fir_xlat's staging)

using nsh::fma2;
using nsh::nf4;
using nsh::crot;
using nsh::phasor;
using nsh::virt;

__device__ __forceinline__ void rotate_one(const float2* in, float2* out, int64_t i, uint64_t inc, uint64_t first)
{
    out[i] = crot(in[i], phasor((first + (uint64_t)i) * inc));
}

// vec != 0: samples [head, head + 2 nv) as 16-byte pairs (in + head and out + head are 16-byte
// aligned), sample 0 (head = 1) and sample n - 1 (odd remainder) by lanes 0 and 1 of workgroup 0.
// vec == 0: every sample on the 8-byte path.
__global__ __launch_bounds__(kBlock) void k_rotate(const float2* in, float2* out, int64_t n, uint64_t inc, uint64_t first,
                                                   float2 step, int head, int64_t nv, int vec)
{
    if (!vec) {
        const int64_t stride = (int64_t)gridDim.x * kBlock;
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) rotate_one(in, out, i, inc, first);
        return;
    }
    const nf4* vin = reinterpret_cast<const nf4*>(in + head);
    nf4* vout = reinterpret_cast<nf4*>(out + head);
    const int64_t gstep = (int64_t)gridDim.x * kBlock * kUnroll;
    for (int64_t base = (int64_t)blockIdx.x * kBlock * kUnroll + threadIdx.x; base < nv; base += gstep) {
        nf4 v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t i = base + (int64_t)u * kBlock;
            if (i < nv) v[u] = __builtin_nontemporal_load(vin + i);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t i = base + (int64_t)u * kBlock;
            if (i < nv) {
                const float2 w0 = phasor((first + (uint64_t)head + 2 * (uint64_t)i) * inc);
                const float2 w1 = crot(w0, step);
                const float2 a = crot(make_float2(v[u].x, v[u].y), w0);
                const float2 b = crot(make_float2(v[u].z, v[u].w), w1);
                const nf4 y = { a.x, a.y, b.x, b.y };
                __builtin_nontemporal_store(y, vout + i);
            }
        }
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0 && head) rotate_one(in, out, 0, inc, first);
        if (threadIdx.x == 1 && ((n - head) & 1)) rotate_one(in, out, n - 1, inc, first);
    }
}

template <int R, int S>
__global__ __launch_bounds__(kBlock) void k_fir_xlat(const float2* __restrict__ in,
                                                     const float2* __restrict__ hist_in,
                                                     float2* __restrict__ hist_out,
                                                     float2* __restrict__ out,
                                                     const float* __restrict__ grev, // g[q] = h[L-1-q], L + 8 floats
                                                     int L,
                                                     int D,
                                                     int a,  // LDS entry of sample s: s + (s >> a)
                                                     int Lc, // taps per part, a multiple of 8
                                                     int64_t n_out,
                                                     uint64_t inc,
                                                     uint64_t first,
                                                     float2 step)
{
    extern __shared__ __attribute__((aligned(16))) float2 xs[];
    constexpr int T = kBlock * R / S; // outputs per workgroup
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int part = wave % S;                     // uniform per wave
    const int grp = (wave / S) * 64 + (tid & 63);  // the lane's outputs: grp R + r
    const int64_t n_in = n_out * D;
    const int64_t m0 = (int64_t)blockIdx.x * T;
    const int64_t g0 = m0 * D - (L - 1);           // stream sample (of this call) at window position 0
    const int count = (T - 1) * D + L;

    // stage and rotate: nsh::stage_window's loop (nsh_stream_tile.hpp) with the rotation in place of
    // its put: a lane's two neighbouring samples take one sincospif and the step phasor. Kept apart,
    // like the history loop below: through the shared pieces the prologue and the first and last
    // windows' code came out in another order, and D = 64 measured 1 to 2 % slower
    // (profiles/stream_refactor_ab.log). The direct loads are plain ones, not ld_nt.
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
                    const float2 w0 = phasor((first + (uint64_t)(g0 + i)) * inc);
                    const float2 w1 = crot(w0, step);
                    xs[i + (i >> a)] = crot(x0[u], w0);
                    if (i + 1 < count) xs[(i + 1) + ((i + 1) >> a)] = crot(x1[u], w1);
                }
            }
        }
    };
    if (g0 >= 0 && g0 + count <= n_in)
        stage([&](int i) { return in[g0 + i]; });
    else
        stage([&](int i) { return virt(in, hist_in, g0 + i, n_in, L); });
    if (blockIdx.x == 0) { // history for the next call: the L-1 raw samples before in[n_in]
        for (int j = tid; j < L - 1; j += kBlock) hist_out[j] = virt(in, hist_in, n_in - (L - 1) + j, n_in, L);
    }
    __syncthreads();

    float2 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = make_float2(0.f, 0.f);

    const int qlo = part * Lc, qhi = min(L, qlo + Lc); // this wave's reversed taps [qlo, qhi)
    const int RD = R * D;
    const int pbase = grp * (RD + (RD >> a));
    if (qlo < qhi) {
        const int jend = (R - 1) * D + qhi;
        for (int jb = qlo; jb < jend; jb += 8) { // span samples jb .. jb + 7 (jb a multiple of 8)
            float2 x[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int j = jb + i;
                x[i] = xs[pbase + j + (j >> a)];
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int q0 = jb - r * D; // uniform
                if (q0 >= qlo && q0 + 8 <= qhi) {
                    float g[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) g[i] = grev[q0 + i];
#pragma unroll
                    for (int i = 0; i < 8; ++i) fma2(acc[r], g[i], x[i]);
                } else if (q0 + 8 > qlo && q0 < qhi) { // the part's edges: tap by tap, none outside
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int q = q0 + i;
                        if (q >= qlo && q < qhi) fma2(acc[r], grev[q], x[i]);
                    }
                }
            }
        }
    }
    if constexpr (S > 1) { // partial sums of parts 1 .. S-1 through LDS, added in part order
        __syncthreads();   // every wave is done with the window
        if (part > 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) xs[(part - 1) * T + grp * R + r] = acc[r];
        }
        __syncthreads();
        if (part == 0) {
            for (int p = 1; p < S; ++p) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float2 v = xs[(p - 1) * T + grp * R + r];
                    acc[r].x += v.x;
                    acc[r].y += v.y;
                }
            }
        }
    }
    if (part == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t m = m0 + (int64_t)grp * R + r;
            if (m < n_out) out[m] = acc[r];
        }
    }
}

struct xlat_plan : nsh::stream_plan { // tile: outputs per workgroup T; buf: the reversed taps
    int L = 0, D = 0;
    int R = 0, S = 0;
    int a = 0, Lc = 0;
    uint64_t inc = 0;
    float2 step = { 1.f, 0.f };
    // the instantiation's launcher (pick)
    void (*launch)(const xlat_plan*, const float2*, const float2*, float2*, float2*, int64_t, uint64_t, unsigned,
                   hipStream_t) = nullptr;
};

int phase_inc(double t, uint64_t* inc)
{
    if (!std::isfinite(t)) return -1;
    const double f = std::fmod(t, 1.0);                       // exact, sign of t, |f| < 1
    const double r = std::nearbyint(std::ldexp(std::fabs(f), 64)); // exact scaling, then to nearest (ties to even)
    const uint64_t u = r >= 18446744073709551616.0 ? 0 : (uint64_t)r;
    *inc = f < 0 ? (uint64_t)0 - u : u;
    return 0;
}

float2 step_phasor(uint64_t inc)
{
    const double th = 2.0 * M_PI * std::ldexp((double)(int64_t)inc, -64); // signed: the short way round
    return make_float2((float)std::cos(th), (float)std::sin(th));
}

template <int R, int S>
void launch_xlat(const xlat_plan* p, const float2* in, const float2* hin, float2* hout, float2* out, int64_t n_out,
                 uint64_t first, unsigned grid, hipStream_t s)
{
    nsh::launch((k_fir_xlat<R, S>), dim3(grid), dim3(kBlock), (uint32_t)p->lds, s, in, hin, hout, out,
                (const float*)p->buf, p->L, p->D, p->a, p->Lc, n_out, p->inc, first, p->step);
}

template <int R, int S>
void pick(xlat_plan* p)
{
    p->R = R, p->S = S;
    p->fn = (const void*)k_fir_xlat<R, S>;
    p->launch = launch_xlat<R, S>;
}

} // namespace

extern "C" {

int nsh_phase_inc(double turns_per_sample, uint64_t* inc)
{
    if (!inc) return nsh::fail_msg("nsh_phase_inc: null pointer");
    if (phase_inc(turns_per_sample, inc)) return nsh::fail_msg("nsh_phase_inc: the frequency must be finite");
    return 0;
}

int nsh_rotate_cc(const float* in, float* out, int64_t n, uint64_t phase_inc, uint64_t first_index, void* stream)
{
    nsh::launch_events_guard timing_guard; // an armed event pair never outlives this call
    if (n > 0 && (!in || !out)) return nsh::fail_msg("nsh_rotate_cc: null pointer");
    if (n <= 0) return 0;
    const bool vec = (uintptr_t)in % 16 == (uintptr_t)out % 16;
    const int head = vec && (uintptr_t)in % 16 != 0 ? 1 : 0; // 8-byte aligned: one sample to the 16-byte slot
    const int64_t nv = vec ? (n - head) / 2 : 0;
    int64_t g = vec ? (nv + (int64_t)kBlock * kUnroll - 1) / ((int64_t)kBlock * kUnroll) : (n + kBlock - 1) / kBlock;
    g = std::min<int64_t>(std::max<int64_t>(g, 1), vec ? 65536 : 4096);
    nsh::launch(k_rotate, dim3((unsigned)g), dim3(kBlock), 0, nsh::S(stream), (const float2*)in, (float2*)out, n, phase_inc,
                first_index, step_phasor(phase_inc), head, nv, vec ? 1 : 0);
    NSH_CK_LAUNCH("nsh_rotate_cc");
    return 0;
}

int nsh_fir_xlat_plan_create(int dev, const float* taps_host, int ntaps, int decim, double freq_norm, void** plan)
{
    if (!taps_host || !plan) return nsh::fail_msg("nsh_fir_xlat_plan_create: null pointer");
    if (ntaps < 1 || ntaps > 1024) return nsh::fail_msg("nsh_fir_xlat_plan_create: ntaps must be in [1, 1024]");
    if (decim < 1 || decim > 64) return nsh::fail_msg("nsh_fir_xlat_plan_create: decimation must be in [1, 64]");
    uint64_t inc = 0;
    if (phase_inc(-freq_norm, &inc)) return nsh::fail_msg("nsh_fir_xlat_plan_create: the frequency must be finite");
    NSH_CK(hipSetDevice(dev));
    auto p = std::make_unique<xlat_plan>();
    p->dev = dev;
    p->L = ntaps;
    p->hist = ntaps - 1;
    p->D = decim;
    p->inc = inc;
    p->step = step_phasor(inc);
    if (decim <= 4)
        pick<8, 1>(p.get());
    else if (decim <= 8)
        pick<4, 1>(p.get());
    else if (decim <= 16)
        pick<4, 2>(p.get());
    else if (decim <= 32)
        pick<4, 4>(p.get());
    else
        pick<2, 4>(p.get());
    p->tile = kBlock * p->R / p->S;
    p->kernel = "k_fir_xlat<" + std::to_string(p->R) + "," + std::to_string(p->S) + ">";
    const int RD = p->R * decim;
    while (RD % (2 << p->a) == 0) ++p->a; // 2^a: the largest power of two in R D (R is even: a >= 1)
    p->Lc = ((ntaps + p->S - 1) / p->S + 7) / 8 * 8;
    // the window, the 8-sample blocks' overrun past the last lane's span, then the padding
    const int wn = p->tile * decim + ntaps + 8;
    p->lds = (size_t)(wn + (wn >> p->a) + 1) * sizeof(float2);
    // at most 110 KiB (D = 63, L = 1024: a = 1), within the CU's 160 KiB
    std::vector<float> grev((size_t)ntaps + 8, 0.f);
    for (int q = 0; q < ntaps; ++q) grev[q] = taps_host[ntaps - 1 - q];
    if (const int rc = p->upload(grev.data(), grev.size() * sizeof(float), "nsh_fir_xlat_plan_create")) return rc;
    *plan = p.release();
    return 0;
}

int nsh_fir_xlat_plan_destroy(void* plan)
{
    delete static_cast<xlat_plan*>(plan);
    return 0;
}

int nsh_fir_xlat_phase_inc(void* plan, uint64_t* inc)
{
    if (!plan || !inc) return nsh::fail_msg("nsh_fir_xlat_phase_inc: null pointer");
    *inc = static_cast<xlat_plan*>(plan)->inc;
    return 0;
}

int nsh_fir_xlat_tile(void* plan) { return plan ? static_cast<xlat_plan*>(plan)->tile : 0; }
const char* nsh_fir_xlat_kernel(void* plan) { return plan ? static_cast<xlat_plan*>(plan)->kernel.c_str() : ""; }

int nsh_fir_xlat_ccf(void* plan, const float* in, const float* hist_in, float* hist_out, float* out, int64_t n_out,
                     uint64_t first_index, void* stream)
{
    nsh::launch_events_guard timing_guard; // the armed event pair never outlives this call
    auto* p = static_cast<xlat_plan*>(plan);
    unsigned grid = 0;
    const int rc = nsh::check_stream_call("nsh_fir_xlat_ccf", p, in, hist_in, hist_out, out, n_out, INT64_MAX / 64, "ntaps-1",
                                          "outputs", &grid);
    if (rc || !grid) return rc;
    p->launch(p, (const float2*)in, (const float2*)hist_in, (float2*)hist_out, (float2*)out, n_out, first_index, grid,
              nsh::S(stream));
    NSH_CK_LAUNCH("nsh_fir_xlat_ccf");
    return 0;
}

} // extern "C"
