// libnsh_hip.so: pfb_arb_resampler_ccf, resample by an arbitrary rate r (GNU Radio's
// pfb_arb_resampler: a bank of F polyphase filters and their derivative filters, the output taken
// from filter j and moved by mu times derivative filter j), on an exact integer phase.
//
//   step = round(F / r 2^32) filter steps per output (Q32.32), pos(n) = phase + n step,
//   k = pos >> 32, i = k div F, j = k mod F, mu = float((pos & 0xffffffff) >> 8) 2^-24
//   y[n] = sum_{q : j + q F < L} (h[j + q F] + mu d[j + q F]) x[i - q],   d[k] = fl32(h[k+1] - h[k]), d[L-1] = 0
//
// F a power of two in [2, 64], 1 <= L <= 2048, Q = ceil(L / F) taps per filter, 1/64 <= r <= 64. The
// host arithmetic (step, and the span of a call: outputs, inputs consumed, next phase) is
// newsched_amd/csrc/nsh_arb_span.hpp. The state between calls is the phase (on the host) and the history: the
// Q-1 raw samples before in[0].
//
//   k_arb<R,P>   one launch per call. A 256-thread workgroup makes T consecutive outputs, R per lane
//                (lane w: outputs w, w + 256, ... of the tile), T <= 256 R chosen per plan so that the
//                tile's window, inputs i(n0) - (Q-1) .. i(n0 + T-1), holds at most 8192 samples.
//     index      Per output, in 64 bits without a 128-bit product: with step = si 2^32 + sf and
//                phase = pi 2^32 + pf, lo = pf + n sf (n < 2^31, so below 2^63 + 2^32),
//                k = pi + n si + (lo >> 32), fraction = lo & 0xffffffff.
//     stage      The window by nsh::stage_window (nsh_stream_tile.hpp), with 8-byte non-temporal
//                loads (ring pointers are only 8-byte aligned). The taps go to LDS as interleaved
//                (h, d) pairs, one ds_read_b64 per tap: tap k = j + q F at entry
//                q P + j + (j >> 5) pad, P = F + pad.
//     FIR        q ascending, w = fmaf(mu, d, h), then one FMA per component: acc = fmaf(w, x, acc).
//                The order is fixed per output, whatever the tile and the call it falls into. Taps
//                j + q F >= L (the padding up to Q F) are skipped, never multiplied: only the last q
//                can hold one, and it takes a per-output test.
//     banks      A ds_read_b64 serves lanes 0-31 and 32-63 separately, bank pair = entry mod 32.
//                Taps: all lanes read the same q, so the bank pair is that of j (plus a common
//                rotation): up to F = 32 different j lie on different bank pairs and equal j are a
//                broadcast: conflict-free with pad = 0. With F = 64, j and j + 32 would share a bank
//                pair; the plan moves the upper half of each row by the pad in [0, 31] with the
//                smallest worst-case multiplicity over 32 consecutive outputs at sampled phases
//                (two entries on a bank pair can remain: 64 filters, 32 bank pairs). This choice and
//                the next are nsh_stream_layout.hpp's arb_layout_of.
//                Samples, r >= 1 (k_arb<R,1>): consecutive outputs read samples that never
//                decrease and rise by at most one per lane: at most 32 consecutive samples (equal
//                ones are a broadcast), conflict-free with the image packed, as in k_resamp<8,1>.
//                r < 1 (k_arb<R,0>): the lanes are 1/r samples apart, and take k_fir_xlat's shift
//                padding: sample s at entry s + (s >> a), the plan picks the a in {31 (none), 6, ..., 1}
//                with the smallest worst-case multiplicity at sampled phases (ties: the larger a).
//     store      Through LDS: after a barrier the lanes write their outputs over the sample image at
//                their place in the tile, and nsh::store_tile reads the tile back linearly (T is even).
//     history    Workgroup 0 writes hist_out: the Q-1 raw samples before in[c], c the inputs the call
//                consumes. An advancing call (n_out = 0) is this workgroup alone.
//   Instantiations: <4,1> for r >= 1 (T = 1024); <4,0>, <2,0>, <1,0> for r < 1 by the T the window allows.
//   Accuracy: fp32 throughout. Non-finite samples propagate by IEEE arithmetic: output n is
//   non-finite exactly when one of its products holds the sample.
#include "nsh_stream_tile.hpp"

#include "nsh_arb_span.hpp"

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

namespace {

constexpr int kBlock = nsh::kStreamBlock;
constexpr int kStage = 8; // sample pairs a lane loads before it stores the first
constexpr int kMaxWindow = nsh::kStreamMaxTile;

using nsh::fma2;
using nsh::ld_nt;
using nsh::virt;

struct arb_args {
    uint64_t phase;
    uint32_t step_i, step_f; // step = step_i 2^32 + step_f
    int64_t n_in, n_out, consumed;
    int L, F, fshift, Q;
    int T;     // outputs per workgroup
    int wmax;  // entries of the sample image: no window is longer
    int a;     // !kLinear: LDS entry of sample s is s + (s >> a)
    int pad, P; // tap k = j + q F at pair entry q P + j + (j >> 5) pad
    int hs_at; // first float2 entry of the taps in LDS
    int vec;   // 16-byte stores
};

template <int R, bool kLinear>
__global__ __launch_bounds__(kBlock) void k_arb(const float2* __restrict__ in,
                                                const float2* __restrict__ hist_in,
                                                float2* __restrict__ hist_out,
                                                float2* __restrict__ out,
                                                const float2* __restrict__ taps, // the (h, d) image, Q P pairs
                                                const arb_args p)
{
    extern __shared__ __attribute__((aligned(16))) float2 xs[];
    float2* hs = xs + p.hs_at;

    const int a = p.a;
    const auto entry = [a](int s) { return kLinear ? s : s + (s >> a); };
    const int tid = threadIdx.x;
    const int H = p.Q - 1;

    // nsh::store_history's loop with two bounds: the history ends at in[consumed], the input at in[n_in]
    if (blockIdx.x == 0) {
        for (int j = tid; j < H; j += kBlock) hist_out[j] = virt(in, hist_in, p.consumed - H + j, p.n_in, p.Q);
    }
    if (p.n_out <= 0) return; // an advancing call

    const uint64_t pf = p.phase & 0xffffffffull, pi = p.phase >> 32;
    // k(n) and the fraction of pos(n), n < 2^31
    const auto index = [&](int64_t n, uint32_t& frac) {
        const uint64_t lo = pf + (uint64_t)n * p.step_f;
        frac = (uint32_t)lo;
        return pi + (uint64_t)n * p.step_i + (lo >> 32);
    };
    const int64_t n0 = (int64_t)blockIdx.x * p.T; // the tile's first output
    const int64_t n_last = (n0 + p.T < p.n_out ? n0 + p.T : p.n_out) - 1;
    uint32_t unused;
    const int64_t i0 = (int64_t)(index(n0, unused) >> p.fshift);
    const int64_t i1 = (int64_t)(index(n_last, unused) >> p.fshift);
    const int64_t g0 = i0 - H; // stream sample (of this call) at window position 0
    const int count = i1 - i0 + p.Q < p.wmax ? (int)(i1 - i0) + p.Q : p.wmax;

    const auto put = [&](int i, float2 x0, float2 x1) {
        xs[entry(i)] = x0;
        if (i + 1 < count) xs[entry(i + 1)] = x1;
    };
    const auto stage = [&](auto load) { nsh::stage_window<kBlock, kStage>(count, tid, load, put); };
    if (g0 >= 0 && g0 + count <= p.n_in)
        stage([&](int i) { return ld_nt(in + g0 + i); });
    else
        stage([&](int i) { return virt(in, hist_in, g0 + i, p.n_in, p.Q); });
    for (int i = tid; i < p.Q * p.P; i += kBlock) hs[i] = taps[i];
    __syncthreads();

    const int qall = p.L >> p.fshift; // taps every filter has: q < qall
    float2 acc[R];
    float mu[R];
    int s0[R], t0[R], j[R];
#pragma unroll
    for (int t = 0; t < R; ++t) {
        // a lane past the tile's end computes the last output again and stores nothing
        const int64_t n = n0 + tid + t * kBlock < n_last ? n0 + tid + t * kBlock : n_last;
        uint32_t frac;
        const uint64_t k = index(n, frac);
        j[t] = (int)(k & (uint64_t)(p.F - 1));
        t0[t] = j[t] + (j[t] >> 5) * p.pad;
        s0[t] = min((int)((int64_t)(k >> p.fshift) - i0), count - p.Q) + H; // window position of x[i(n)]
        mu[t] = (float)(frac >> 8) * 0x1p-24f;
        acc[t] = make_float2(0.f, 0.f);
    }
#pragma unroll 2
    for (int q = 0; q < qall; ++q) {
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const float2 hd = hs[t0[t] + q * p.P];
            const float2 x = xs[entry(s0[t] - q)]; // both reads before the first use
            fma2(acc[t], __builtin_fmaf(mu[t], hd.y, hd.x), x);
        }
    }
    if (qall < p.Q) { // the last, partial row of taps
#pragma unroll
        for (int t = 0; t < R; ++t) {
            if (j[t] + qall * p.F < p.L) {
                const float2 hd = hs[t0[t] + qall * p.P];
                const float2 x = xs[entry(s0[t] - qall)]; // both reads before the first use
                fma2(acc[t], __builtin_fmaf(mu[t], hd.y, hd.x), x);
            }
        }
    }
    __syncthreads(); // every lane is done with the samples: the tile's outputs take their place
#pragma unroll
    for (int t = 0; t < R; ++t)
        if (tid + t * kBlock < p.T) xs[tid + t * kBlock] = acc[t];
    __syncthreads();

    nsh::store_tile<kBlock>(xs, out, n0, p.T, p.n_out, p.vec, tid);
}

struct arb_plan : nsh::stream_plan { // tile: outputs per workgroup T; buf: the (h, d) image
    int L = 0, F = 0, fshift = 0, Q = 0;
    uint64_t step = 0;
    int R = 0, wmax = 0;
    int a = 31, pad = 0, P = 0, hs_at = 0;
    // the instantiation's launcher (pick)
    void (*launch)(const arb_plan*, const float2*, const float2*, float2*, float2*, const arb_args&, unsigned,
                   hipStream_t) = nullptr;
};

template <int R, bool kLinear>
void launch_arb(const arb_plan* p, const float2* in, const float2* hin, float2* hout, float2* out, const arb_args& args,
                unsigned grid, hipStream_t s)
{
    nsh::launch((k_arb<R, kLinear>), dim3(grid), dim3(kBlock), (uint32_t)p->lds, s, in, hin, hout, out,
                (const float2*)p->buf, args);
}

template <int R, bool kLinear>
void pick(arb_plan* p)
{
    p->R = R;
    p->fn = (const void*)k_arb<R, kLinear>;
    p->launch = launch_arb<R, kLinear>;
    p->kernel = "k_arb<" + std::to_string(R) + (kLinear ? ",1>" : ",0>");
}

} // namespace

extern "C" {

int nsh_arb_step(double rate, int nfilt, uint64_t* step)
{
    if (!step) return nsh::fail_msg("nsh_arb_step: null pointer");
    if (nsh_arb::filt_shift(nfilt) < 0) return nsh::fail_msg("nsh_arb_step: nfilt must be a power of two in [2, 64]");
    if (!nsh_arb::rate_ok(rate)) return nsh::fail_msg("nsh_arb_step: rate must be finite and in [1/64, 64]");
    *step = nsh_arb::step_of(rate, nfilt);
    return 0;
}

int nsh_arb_span(uint64_t step, int nfilt, uint64_t phase, int64_t n_in, int64_t want_out, int64_t* n_out,
                 int64_t* n_consumed, uint64_t* phase_next)
{
    if (!n_out || !n_consumed || !phase_next) return nsh::fail_msg("nsh_arb_span: null pointer");
    const int fshift = nsh_arb::filt_shift(nfilt);
    if (fshift < 0) return nsh::fail_msg("nsh_arb_span: nfilt must be a power of two in [2, 64]");
    if (!nsh_arb::step_ok(step, fshift)) return nsh::fail_msg("nsh_arb_span: step is not that of a rate in [1/64, 64]");
    if (n_in < 0 || n_in > nsh_arb::kMaxItems || want_out < 0 || want_out > nsh_arb::kMaxItems)
        return nsh::fail_msg("nsh_arb_span: n_in and want_out must be in [0, 2^31 - 1]");
    const nsh_arb::span s = nsh_arb::span_of(step, fshift, phase, n_in, want_out);
    *n_out = s.n_out;
    *n_consumed = s.n_consumed;
    *phase_next = s.phase_next;
    return 0;
}

int nsh_arb_plan_create(int dev, const float* taps_host, int ntaps, int nfilt, double rate, void** plan)
{
    if (!taps_host || !plan) return nsh::fail_msg("nsh_arb_plan_create: null pointer");
    if (nsh_arb::filt_shift(nfilt) < 0) return nsh::fail_msg("nsh_arb_plan_create: nfilt must be a power of two in [2, 64]");
    if (ntaps < 1 || ntaps > 2048) return nsh::fail_msg("nsh_arb_plan_create: ntaps must be in [1, 2048]");
    if (!nsh_arb::rate_ok(rate)) return nsh::fail_msg("nsh_arb_plan_create: rate must be finite and in [1/64, 64]");
    NSH_CK(hipSetDevice(dev));
    auto p = std::make_unique<arb_plan>();
    p->dev = dev;
    p->L = ntaps;
    p->F = nfilt;
    p->fshift = nsh_arb::filt_shift(nfilt);
    p->Q = (ntaps + nfilt - 1) / nfilt;
    p->hist = p->Q - 1;
    p->step = nsh_arb::step_of(rate, nfilt);
    const int fshift = p->fshift;
    const uint64_t step = p->step, unit = 1ull << (32 + fshift); // one input sample
    const nsh::arb_layout lay = nsh::arb_layout_of(step, fshift);
    // T outputs span at most floor((T-1) step / unit) + 1 inputs after the first one's
    const auto window = [&](int T) { return (int)(((uint64_t)(T - 1) * step) >> (32 + fshift)) + 1 + p->Q; };
    // the largest T the window allows: (T-1) step < (kMaxWindow - Q) unit, at least 111 (r = 1/64, Q = 1024)
    const uint64_t t_fit = ((uint64_t)(kMaxWindow - p->Q) * unit - 1) / step + 1;
    if (lay.linear)
        pick<4, true>(p.get());
    else if (t_fit >= 4 * kBlock)
        pick<4, false>(p.get());
    else if (t_fit >= 2 * kBlock)
        pick<2, false>(p.get());
    else
        pick<1, false>(p.get());
    p->tile = (int)std::min<uint64_t>((uint64_t)p->R * kBlock, t_fit) & ~1; // even: 16-byte stores
    p->wmax = window(p->tile);
    if (p->wmax > kMaxWindow) return nsh::fail_msg("nsh_arb_plan_create: internal: window too long");
    p->a = lay.a, p->pad = lay.pad;
    p->P = nfilt + p->pad;
    // the sample image (the tile's outputs take its place later), then the taps, 16-byte aligned
    p->hs_at = (std::max(p->wmax + (p->wmax >> p->a) + 1, p->tile) + 1) / 2 * 2;
    p->lds = ((size_t)p->hs_at + (size_t)p->Q * p->P) * sizeof(float2);
    // at most 96 KiB of samples (8192 at a = 1) and 24 KiB of taps (F = 64, pad = 31), within the CU's 160 KiB
    std::vector<float> d((size_t)ntaps);
    nsh_arb::diff_taps(taps_host, ntaps, d.data());
    std::vector<float2> host((size_t)p->Q * p->P, make_float2(0.f, 0.f));
    for (int k = 0; k < ntaps; ++k) {
        const int j = k & (nfilt - 1), q = k >> fshift;
        host[(size_t)q * p->P + j + (j >> 5) * p->pad] = make_float2(taps_host[k], d[k]);
    }
    if (const int rc = p->upload(host.data(), host.size() * sizeof(float2), "nsh_arb_plan_create")) return rc;
    *plan = p.release();
    return 0;
}

int nsh_arb_plan_destroy(void* plan)
{
    delete static_cast<arb_plan*>(plan);
    return 0;
}

int nsh_arb_tile(void* plan) { return plan ? static_cast<arb_plan*>(plan)->tile : 0; }
const char* nsh_arb_kernel(void* plan) { return plan ? static_cast<arb_plan*>(plan)->kernel.c_str() : ""; }
int nsh_arb_history(void* plan) { return plan ? static_cast<arb_plan*>(plan)->hist : 0; }
int nsh_arb_plan_step(void* plan, uint64_t* step)
{
    if (!plan || !step) return nsh::fail_msg("nsh_arb_plan_step: null pointer");
    *step = static_cast<arb_plan*>(plan)->step;
    return 0;
}

int nsh_arb_resamp_ccf(void* plan, const float* in, int64_t n_in, const float* hist_in, float* hist_out, float* out,
                       int64_t n_out, uint64_t phase, void* stream)
{
    nsh::launch_events_guard timing_guard; // the armed event pair never outlives this call
    auto* p = static_cast<arb_plan*>(plan);
    // what needs no plan comes first, as in nsh::check_stream_call
    if (hist_in && hist_in == hist_out) return nsh::fail_msg("nsh_arb_resamp_ccf: hist_out must not alias hist_in");
    if (n_in > 0 && (!in || (n_out > 0 && !out))) return nsh::fail_msg("nsh_arb_resamp_ccf: null input or output");
    if (n_in > nsh_arb::kMaxItems || n_out > nsh_arb::kMaxItems)
        return nsh::fail_msg("nsh_arb_resamp_ccf: n_in and n_out must not exceed 2^31 - 1");
    if (!p) return nsh::fail_msg("nsh_arb_resamp_ccf: null plan");
    if (n_in <= 0) return 0;
    if (n_out < 0) n_out = 0;
    if (!hist_out && p->Q > 1) return nsh::fail_msg("nsh_arb_resamp_ccf: hist_out is required (ceil(ntaps / nfilt) - 1 samples)");
    const nsh_arb::span s = nsh_arb::span_of(p->step, p->fshift, phase, n_in, n_out);
    if (s.n_out < n_out) return nsh::fail_msg("nsh_arb_resamp_ccf: n_out is more than n_in inputs hold from this phase (nsh_arb_span)");
    if (n_out == 0 && p->Q == 1) return 0; // an advancing call without a history: nothing to write
    arb_args a;
    a.phase = phase;
    a.step_i = (uint32_t)(p->step >> 32);
    a.step_f = (uint32_t)p->step;
    a.n_in = n_in;
    a.n_out = n_out;
    a.consumed = s.n_consumed;
    a.L = p->L, a.F = p->F, a.fshift = p->fshift, a.Q = p->Q;
    a.T = p->tile, a.wmax = p->wmax, a.a = p->a, a.pad = p->pad, a.P = p->P, a.hs_at = p->hs_at;
    a.vec = nsh::store_vec16(out, p->tile);
    const int64_t grid = std::max<int64_t>((n_out + p->tile - 1) / p->tile, 1);
    p->launch(p, (const float2*)in, (const float2*)hist_in, (float2*)hist_out, (float2*)out, a, (unsigned)grid,
              nsh::S(stream));
    NSH_CK_LAUNCH("nsh_arb_resamp_ccf");
    return 0;
}

} // extern "C"
