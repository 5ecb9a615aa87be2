// libnsh_hip.so: pfb_channelizer_ccf, the critically sampled M-channel polyphase filterbank.
//
//   y[m][c] = sum_{k<L} h[k] x[mM - k] exp(+j 2 pi c k / M)         (0 <= c < M, GNU Radio's order)
//           = sum_{p<M} u_p[m] exp(+j 2 pi c p / M),   u_p[m] = sum_{q<Q} h[p + qM] x[(m-q)M - p]
//
// with k = p + qM and Q = ceil(L / M): M branch FIRs of Q real taps, then an unnormalised inverse
// DFT across the branches. M is a power of two in [2, 64], L <= 1024, Q <= 32.
//
//   k_pfb<M>   one launch per call. A 256-thread workgroup makes T = 256 R / M time steps, R = 8
//              steps per lane: T M = 2048 samples. The (Q-1) M halo it re-reads is 7 M / 2048 of
//              its tile at Q = 8 (5.5 % at M = 16, 22 % at M = 64), and still the small tile is the
//              faster one: four- and eight-thousand-sample tiles, with two to three workgroups per
//              CU instead of five, measured 6 to 49 % slower.
//     stage    The window of the tile, rows of M samples: row j holds the stream samples of time
//              step m0 - (Q-1) + j in stream order, x[(m0-Q+1+j) M - (M-1) + c] in column c, so
//              branch p reads column M-1-p. (T+Q-1) M samples, each read from HBM once per
//              workgroup with 8-byte non-temporal loads (ring pointers are only 8-byte aligned),
//              in the order of nsh::stage_window (nsh_stream_tile.hpp), in a loop of the kernel's own.
//              The taps go to LDS as hs[q][p], zero-padded to a multiple of 4 rows.
//     FIR      Lane (tg, p) = (tid / M, tid mod M) keeps the R consecutive time steps tg R + t of
//              branch p. It walks the taps in chunks of 4 and
//              holds the R + 3 rows the chunk needs in registers; the next chunk moves R - 1 of
//              them up and reads 4 new rows: R + Qp - 1 ds_read_b64 for R Q MACs (Qp = Q rounded
//              up to 4). Taps k >= L (the padding up to Qp M) are skipped, never multiplied: a
//              chunk that holds one takes the path with a per-lane test (0 x NaN would poison a
//              time step whose window does not hold the sample).
//     banks    A ds_read_b64 serves lanes 0-31 and 32-63 separately, bank pair = entry mod 32. Lanes
//              along p read consecutive entries of one row. M >= 32: the 32 lanes of a group read
//              32 consecutive entries of one row: conflict-free with rows packed, row j at entry
//              j M. M < 32: a group holds 32 / M time groups tg whose rows are R apart; with rows
//              packed they would sit R M entries apart, a multiple of 16: on the same banks. The image
//              therefore leaves one row free after every R: row j at entry (j + (j >> 3)) M, so
//              neighbouring time groups are 9 M entries apart whatever row of their window they
//              read, and 9 tg mod (32 / M) takes every value once: 32 different bank pairs.
//              tests/test_pfb_layout.py recomputes this for every instantiation.
//     IDFT     Radix-2 decimation in frequency across the M lanes of a time step, log2 M stages of
//              one lane exchange (xor M/2, M/4, ..., 1) each: the lane without the stage's bit keeps
//              a + b, the one with it (a_low - a_high) w, w = exp(+j 2 pi (p mod half) / (2 half))
//              from a table computed in double on the host (exact constants, no runtime sincos).
//              The last stage's twiddle is 1 and is not multiplied. Lane p ends with channel
//              bitrev(p).
//     store    Through a wave-private LDS image (a wave's time steps are its own: no workgroup
//              barrier after staging), written at [step][bitrev(p)] and read back linearly, so a
//              wave stores runs of R/2 M contiguous samples, in two rounds of R/2 steps each (half
//              the image: 10 KiB per workgroup). 16-byte non-temporal stores when out is 16-byte
//              aligned, the 8-byte path otherwise. The image is padded against the bit-reversed
//              writes (ds_write_b64: 16 contiguous lanes, bank pair = entry mod 16): M >= 32 one
//              entry after every 16, M < 32 M entries after every step block of a time group.
//   Accuracy: fp32 throughout. The DFT mixes the branches, so errors are relative to the largest
//   channel of a time step, not to each channel. Non-finite samples propagate by IEEE arithmetic: a
//   NaN in the L-tap window of a time step makes all M channels of that step NaN and no other.
#include "nsh_pfb_geom.hpp"

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

namespace {

constexpr int kStage = 8; // sample pairs a lane loads before it stores the first

using nsh::fma2;
using nsh::ilog2;
using nsh::ld_nt;
using nsh::nf2;
using nsh::nf4;
using nsh::virt;
using nsh::wave_lds_sync;
using nsh::pfb::geom; // the tile and the LDS images (nsh_pfb_geom.hpp), shared with k_pfb_synth
using nsh::pfb::kBlock;
using nsh::pfb::kQC;
using nsh::pfb::kR;
using nsh::pfb::kRounds;

template <int M>
__global__ __launch_bounds__(kBlock) void k_pfb(const float2* __restrict__ in,
                                                const float2* __restrict__ hist_in,
                                                float2* __restrict__ hist_out,
                                                float2* __restrict__ out,
                                                const float* __restrict__ hp,  // hp[q M + p] = h[p + q M], Qp M floats
                                                const float2* __restrict__ tw, // tw[s M + p], log2 M - 1 stages
                                                int L,
                                                int Q,
                                                int Qp, // Q rounded up to kQC
                                                int64_t n_out,
                                                int vec) // out is 16-byte aligned
{
    using g = geom<M>;
    constexpr int LOG2M = g::LOG2M;
    extern __shared__ __attribute__((aligned(16))) float2 xs[];
    const int rows = g::T + Q - 1;
    float* hs = reinterpret_cast<float*>(xs + g::row_entry(rows));
    float2* ys = reinterpret_cast<float2*>(hs + Qp * M);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p = tid & (M - 1);
    const int tg = tid >> LOG2M;
    const int64_t n_in = n_out * M;
    const int64_t m0 = (int64_t)blockIdx.x * g::T;
    const int64_t g0 = (m0 - (Q - 1)) * M - (M - 1); // stream sample (of this call) at window position 0
    const int count = rows * M;

    // nsh::stage_window's loop, kept apart: the window is whole rows, so count is even and one test
    // serves both loads of a pair. Through the shared loop the compiler made other memory
    // instructions (a 16-byte load split in two, 40 to 110 instructions more per instantiation).
    auto stage = [&](auto load) {
        for (int i0 = 2 * tid; i0 < count; i0 += 2 * kBlock * kStage) {
            float2 x0[kStage], x1[kStage];
#pragma unroll
            for (int u = 0; u < kStage; ++u) {
                const int i = i0 + 2 * kBlock * u; // even, count is even: i + 1 < count too
                x0[u] = i < count ? load(i) : make_float2(0.f, 0.f);
                x1[u] = i < count ? load(i + 1) : make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < kStage; ++u) {
                const int i = i0 + 2 * kBlock * u;
                if (i < count) {
                    const int e = g::row_entry(i >> LOG2M) + (i & (M - 1)); // i and i + 1 share a row
                    xs[e] = x0[u];
                    xs[e + 1] = x1[u];
                }
            }
        }
    };
    if (g0 >= 0 && g0 + count <= n_in)
        stage([&](int i) { return ld_nt(in + g0 + i); });
    else
        stage([&](int i) { return virt(in, hist_in, g0 + i, n_in, L); });
    for (int i = tid; i < Qp * M; i += kBlock) hs[i] = hp[i];
    if (blockIdx.x == 0) nsh::store_history<kBlock>(in, hist_in, hist_out, n_in, L, tid);

    float2 w[LOG2M > 1 ? LOG2M - 1 : 1];
#pragma unroll
    for (int s = 0; s < LOG2M - 1; ++s) w[s] = tw[s * M + p];
    const int qv = (L - p + M - 1) >> LOG2M; // this branch's taps: q < qv
    const int qall = L >> LOG2M;             // taps every branch has: q < qall
    const int col = M - 1 - p;
    const int ch = (int)(__builtin_bitreverse32((unsigned)p) >> (32 - LOG2M));
    float2* yw = ys + wave * g::YW;
    __syncthreads();

    const int trow = tg * kR; // the lane's first time step in the tile
    auto row = [&](int rho) { return xs[g::row_entry(trow + max(rho, 0)) + col]; };

    float2 acc[kR];
#pragma unroll
    for (int t = 0; t < kR; ++t) acc[t] = make_float2(0.f, 0.f);
    // tap q = q0 + dq of time step t meets row t + Q-1 - q = lo + k, k = t + kQC-1 - dq
    int lo = Q - kQC;
    float2 xw[kR + kQC - 1];
#pragma unroll
    for (int k = 0; k < kR + kQC - 1; ++k) xw[k] = row(lo + k);
    for (int q0 = 0; q0 < Qp; q0 += kQC) {
        float h[kQC];
#pragma unroll
        for (int dq = 0; dq < kQC; ++dq) h[dq] = hs[(q0 + dq) * M + p];
        if (q0 + kQC <= qall) {
#pragma unroll
            for (int dq = 0; dq < kQC; ++dq)
#pragma unroll
                for (int t = 0; t < kR; ++t) fma2(acc[t], h[dq], xw[t + kQC - 1 - dq]);
        } else { // the chunk holds taps at or past L: tap by tap, none outside
#pragma unroll
            for (int dq = 0; dq < kQC; ++dq) {
                if (q0 + dq < qv) {
#pragma unroll
                    for (int t = 0; t < kR; ++t) fma2(acc[t], h[dq], xw[t + kQC - 1 - dq]);
                }
            }
        }
        if (q0 + kQC < Qp) { // slide down by kQC rows
            lo -= kQC;
#pragma unroll
            for (int k = kR - 2; k >= 0; --k) xw[k + kQC] = xw[k];
#pragma unroll
            for (int k = 0; k < kQC; ++k) xw[k] = row(lo + k);
        }
    }

    // inverse DFT across the M lanes of each time step
#pragma unroll
    for (int s = 0; s < LOG2M; ++s) {
        const int half = M >> (s + 1);
        const float sgn = (p & half) ? -1.f : 1.f;
#pragma unroll
        for (int t = 0; t < kR; ++t) {
            const float bx = __shfl_xor(acc[t].x, half, 64);
            const float by = __shfl_xor(acc[t].y, half, 64);
            const float tx = __builtin_fmaf(acc[t].x, sgn, bx); // a + b, or (the partner's) a - b
            const float ty = __builtin_fmaf(acc[t].y, sgn, by);
            if (s < LOG2M - 1) {
                acc[t].x = __builtin_fmaf(-ty, w[s].y, tx * w[s].x);
                acc[t].y = __builtin_fmaf(tx, w[s].y, ty * w[s].x);
            } else {
                acc[t].x = tx;
                acc[t].y = ty;
            }
        }
    }

    // the wave's 64 R / M time steps start at mw; its time group tgl holds steps tgl R + t
    const int tgl = lane >> LOG2M;
    const int64_t mw = m0 + wave * (64 / M) * kR;
#pragma unroll
    for (int rd = 0; rd < kRounds; ++rd) {
        wave_lds_sync(); // the reads of the round before
#pragma unroll
        for (int t = 0; t < g::RH; ++t) yw[g::ypos(((tgl * g::RH + t) << LOG2M) + ch)] = acc[rd * g::RH + t];
        wave_lds_sync();
        // image entry e: time group e / (RH M), then RH steps of M channels
        if (vec) {
#pragma unroll
            for (int i = 0; i < g::RH / 2; ++i) {
                const int e = 2 * (64 * i + lane);
                const int blk = e >> (ilog2(g::RH) + LOG2M), rest = e & (g::RH * M - 1);
                const int64_t m = mw + blk * kR + rd * g::RH + (rest >> LOG2M);
                if (m < n_out) {
                    const float2 a = yw[g::ypos(e)], b = yw[g::ypos(e) + 1];
                    const nf4 v = { a.x, a.y, b.x, b.y };
                    __builtin_nontemporal_store(v, reinterpret_cast<nf4*>(out + m * M + (rest & (M - 1))));
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < g::RH; ++i) {
                const int e = 64 * i + lane;
                const int blk = e >> (ilog2(g::RH) + LOG2M), rest = e & (g::RH * M - 1);
                const int64_t m = mw + blk * kR + rd * g::RH + (rest >> LOG2M);
                if (m < n_out) {
                    const float2 a = yw[g::ypos(e)];
                    const nf2 v = { a.x, a.y };
                    __builtin_nontemporal_store(v, reinterpret_cast<nf2*>(out + m * M + (rest & (M - 1))));
                }
            }
        }
    }
}

struct pfb_plan : nsh::stream_plan { // tile: time steps per workgroup T; buf: Qp M taps, then the twiddles
    int L = 0, M = 0, Q = 0, Qp = 0;
    // the instantiation's launcher (setup)
    void (*launch)(const pfb_plan*, const float2*, const float2*, float2*, float2*, int64_t, int, unsigned,
                   hipStream_t) = nullptr;
};

template <int M>
void launch_pfb(const pfb_plan* p, const float2* in, const float2* hin, float2* hout, float2* out, int64_t n_out, int vec,
                unsigned grid, hipStream_t s)
{
    nsh::launch((k_pfb<M>), dim3(grid), dim3(kBlock), (uint32_t)p->lds, s, in, hin, hout, out, (const float*)p->buf,
                (const float2*)((const float*)p->buf + p->Qp * M), p->L, p->Q, p->Qp, n_out, vec);
}

template <int M>
void setup(pfb_plan* p)
{
    using g = geom<M>;
    p->tile = g::T;
    p->fn = (const void*)k_pfb<M>;
    p->launch = launch_pfb<M>;
    p->lds = (size_t)g::row_entry(g::T + p->Q - 1) * sizeof(float2) + (size_t)p->Qp * M * sizeof(float) +
             (size_t)(kBlock / 64) * g::YW * sizeof(float2);
}

} // namespace

extern "C" {

int nsh_pfb_plan_create(int dev, const float* taps_host, int ntaps, int nchans, void** plan)
{
    if (!taps_host || !plan) return nsh::fail_msg("nsh_pfb_plan_create: null pointer");
    if (ntaps < 1 || ntaps > 1024) return nsh::fail_msg("nsh_pfb_plan_create: ntaps must be in [1, 1024]");
    if (nchans < 2 || nchans > 64 || (nchans & (nchans - 1)))
        return nsh::fail_msg("nsh_pfb_plan_create: nchans must be a power of two in [2, 64]");
    const int Q = (ntaps + nchans - 1) / nchans;
    if (Q > 32) return nsh::fail_msg("nsh_pfb_plan_create: at most 32 taps per branch (ceil(ntaps / nchans) <= 32)");
    NSH_CK(hipSetDevice(dev));
    auto p = std::make_unique<pfb_plan>();
    p->dev = dev;
    p->L = ntaps;
    p->hist = ntaps - 1;
    p->M = nchans;
    p->Q = Q;
    p->Qp = (Q + kQC - 1) / kQC * kQC;
    switch (nchans) {
    case 2: setup<2>(p.get()); break;
    case 4: setup<4>(p.get()); break;
    case 8: setup<8>(p.get()); break;
    case 16: setup<16>(p.get()); break;
    case 32: setup<32>(p.get()); break;
    default: setup<64>(p.get()); break;
    }
    p->kernel = "k_pfb<" + std::to_string(nchans) + ">";
    const int M = nchans;
    const size_t ntap = (size_t)p->Qp * M;
    std::vector<float> host(ntap + nsh::pfb::twiddle_floats(M), 0.f);
    for (int k = 0; k < ntaps; ++k) host[k] = taps_host[k]; // hp[q M + p] = h[p + q M]
    nsh::pfb::fill_twiddles(M, host.data() + ntap);
    // at most 37.75 KiB (38 656 bytes, M = 32 with 1024 taps; M = 64 with 1024 taps: 38 400)
    // the twiddles start ntap floats in, a multiple of 8 floats
    if (const int rc = p->upload(host.data(), host.size() * sizeof(float), "nsh_pfb_plan_create")) return rc;
    *plan = p.release();
    return 0;
}

int nsh_pfb_plan_destroy(void* plan)
{
    delete static_cast<pfb_plan*>(plan);
    return 0;
}

int nsh_pfb_tile(void* plan) { return plan ? static_cast<pfb_plan*>(plan)->tile : 0; }
const char* nsh_pfb_kernel(void* plan) { return plan ? static_cast<pfb_plan*>(plan)->kernel.c_str() : ""; }

int nsh_pfb_channelizer_ccf(void* plan, const float* in, const float* hist_in, float* hist_out, float* out, int64_t n_out,
                            void* stream)
{
    nsh::launch_events_guard timing_guard; // the armed event pair never outlives this call
    auto* p = static_cast<pfb_plan*>(plan);
    unsigned grid = 0;
    const int rc = nsh::check_stream_call("nsh_pfb_channelizer_ccf", p, in, hist_in, hist_out, out, n_out, INT64_MAX / 128,
                                          "ntaps-1", "outputs", &grid);
    if (rc || !grid) return rc;
    const int vec = nsh::store_vec16(out, p->tile * p->M);
    p->launch(p, (const float2*)in, (const float2*)hist_in, (float2*)hist_out, (float2*)out, n_out, vec, grid,
              nsh::S(stream));
    NSH_CK_LAUNCH("nsh_pfb_channelizer_ccf");
    return 0;
}

} // extern "C"
