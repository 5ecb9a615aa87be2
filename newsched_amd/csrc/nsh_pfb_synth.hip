// libnsh_hip.so: pfb_synthesizer_ccf, the critically sampled M-channel synthesis filterbank: the
// transpose of pfb_channelizer_ccf (nsh_pfb.hip). Input items X[m][c] of M channels, output stream
//
//   y[n] = sum_{c<M} sum_{m'} X[m'][c] h[n - m' M] exp(+j 2 pi c n / M)          0 <= n - m' M < L
//   v_r[m]     = sum_{c<M} X[m][c] exp(+j 2 pi c r / M)       unnormalised inverse DFT across the channels
//   y[m M + r] = sum_{q<Q, r+qM<L} h[r + q M] v_r[m - q]      M branch FIRs of at most Q = ceil(L / M) taps
//
// M is a power of two in [2, 64], L <= 1024, Q <= 32; no gain of M. The carried history is the Q - 1
// raw items before in[0], (Q-1) M samples.
//
//   k_pfb_synth<M>  one launch per call. Geometry, tap layout, FIR walk and store image are k_pfb's
//              (nsh_pfb_geom.hpp): a 256-thread workgroup makes T = 2048 / M items, 2048 outputs, lane
//              (tg, r) = (tid / M, tid mod M) the R = 8 consecutive items tg R + t of branch r.
//     stage    The window is the T + Q - 1 items from m0 - (Q-1), transformed while it is staged: a
//              lane loads channel p = tid mod M of 8 items 256 / M apart (8-byte non-temporal loads,
//              all issued before the first use; the stream's first and last workgroups through
//              virt()), runs k_pfb's radix-2 network over the M lanes of each item and, holding
//              v_bitrev(p), writes row j of the image at column bitrev(p): the DFT costs no LDS round
//              trip. The exchanges with lane ^ 1, 2, 4, 8 are data-parallel moves in the VALU
//              (xor_lane), only those with lane ^ 16 and ^ 32 go through the LDS crossbar
//              (ds_bpermute): with all log2 M stages there the kernel measured 4 % (M = 16) and 5 to
//              14 % (M = 64) slower. The Q - 1 halo items are transformed again by the next
//              workgroup: 7 M / 2048 of the tile's DFT work at Q = 8 (22 % at M = 64). The halo past
//              the first 2048 samples is staged two items per lane at a time, by the waves it reaches.
//     image    geom<M>::row_entry, with one change at M >= 32: column c of a row lies at c ^ ((c >> 4)
//              & (M / 16 - 1)). The 16 lanes of a ds_write_b64 group hold columns M / 16 apart
//              (bit-reversed), which packed would share M / 16 = 2 or 4 bank pairs (entry mod 16); the
//              xor spreads them over all 16 and permutes only within aligned groups of M / 16
//              columns, so the FIR's reads of 32 consecutive columns stay conflict-free.
//              tests/test_pfb_synth_layout.py recomputes both for every instantiation.
//     FIR      k_pfb's: taps in chunks of 4, the R + 3 rows of a chunk in registers, column r; taps
//              k >= L are skipped, never multiplied.
//     store    k_pfb's wave-private image and read-back with channel = r (no bit reversal): the
//              wave's 512 outputs are one contiguous run, stored in two rounds of 256.
//   Accuracy: fp32 throughout; the DFT mixes the channels, so errors are relative to the loudest. A
//   NaN in any channel of item m' makes exactly the outputs [m' M, m' M + L - 1] NaN.
//   Measured (one MI355X, 2^26 outputs, kernel times, against nsh_copy over the same
//   16 B per output and k_pfb<M> at the same filter): (M, L) = (4, 31) 180 us, 1.07 times the copy and
//   0.98 times k_pfb; (4, 127) 238 us, 1.42 and 1.04; (16, 127) 194 us, 1.15 and 1.00; (64, 127) 210 us,
//   1.25 and 1.01; (64, 511) 265 us, 1.59 and 1.09: the halo's second transform and the two crossbar
//   stages, which k_pfb does not have per halo item.
#include "nsh_pfb_geom.hpp"

#include <memory>
#include <string>
#include <type_traits>
#include <vector>

namespace {

constexpr int kStage = 8; // items a lane loads before it transforms the first
constexpr int kTail = 2;  // the same, past the first kBlock kStage samples of the window

using nsh::fma2;
using nsh::ilog2;
using nsh::ld_nt;
using nsh::nf2;
using nsh::nf4;
using nsh::virt;
using nsh::wave_lds_sync;
using nsh::pfb::geom;
using nsh::pfb::kBlock;
using nsh::pfb::kQC;
using nsh::pfb::kR;

// column c of a window row (see image)
template <int M>
__host__ __device__ constexpr int col_entry(int c)
{
    return M >= 32 ? c ^ ((c >> 4) & (M / 16 - 1)) : c;
}

template <int CTRL>
__device__ __forceinline__ float dpp(float v)
{
    const int i = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, CTRL, 0xf, 0xf, false));
}

// v of lane ^ H. Within a row of 16 lanes by data-parallel moves in the VALU, which leave the LDS
// pipe to the window: quad permutations for 1 and 2; 4 and 8 as two mirrors (lane ^ 7 then ^ 3, lane
// ^ 15 then ^ 7). Across rows through the LDS crossbar.
template <int H>
__device__ __forceinline__ float xor_lane(float v)
{
    constexpr int kQuadXor1 = 0xb1, kQuadXor2 = 0x4e, kQuadXor3 = 0x1b, kRowMirror = 0x140, kRowHalfMirror = 0x141;
    if constexpr (H == 1)
        return dpp<kQuadXor1>(v);
    else if constexpr (H == 2)
        return dpp<kQuadXor2>(v);
    else if constexpr (H == 4)
        return dpp<kQuadXor3>(dpp<kRowHalfMirror>(v));
    else if constexpr (H == 8)
        return dpp<kRowHalfMirror>(dpp<kRowMirror>(v));
    else
        return __shfl_xor(v, H, 64);
}

template <int M, int S, int N>
__device__ __forceinline__ void dft_stage(float2 (&a)[N], const float2* w, int p)
{
    constexpr int LOG2M = ilog2(M);
    if constexpr (S < LOG2M) {
        constexpr int half = M >> (S + 1);
        const int s = S;
        const float sgn = (p & half) ? -1.f : 1.f;
#pragma unroll
        for (int t = 0; t < N; ++t) {
            const float bx = xor_lane<half>(a[t].x);
            const float by = xor_lane<half>(a[t].y);
            const float tx = __builtin_fmaf(a[t].x, sgn, bx); // a + b, or (the partner's) a - b
            const float ty = __builtin_fmaf(a[t].y, sgn, by);
            if (s < LOG2M - 1) {
                a[t].x = __builtin_fmaf(-ty, w[s].y, tx * w[s].x);
                a[t].y = __builtin_fmaf(tx, w[s].y, ty * w[s].x);
            } else {
                a[t].x = tx;
                a[t].y = ty;
            }
        }
        dft_stage<M, S + 1, N>(a, w, p);
    }
}

// Inverse DFT across the M lanes of each of a's N items: radix-2 decimation in frequency, one lane
// exchange per stage (k_pfb's IDFT); lane p ends with element bitrev(p).
template <int M, int N>
__device__ __forceinline__ void lane_dft(float2 (&a)[N], const float2* w, int p)
{
    dft_stage<M, 0, N>(a, w, p);
}

template <int M>
__global__ __launch_bounds__(kBlock) void k_pfb_synth(const float2* __restrict__ in,
                                                      const float2* __restrict__ hist_in,
                                                      float2* __restrict__ hist_out,
                                                      float2* __restrict__ out,
                                                      const float* __restrict__ hp,  // hp[q M + r] = h[r + q M], Qp M floats
                                                      const float2* __restrict__ tw, // tw[s M + p], log2 M - 1 stages
                                                      int L,
                                                      int Q,
                                                      int Qp, // Q rounded up to kQC
                                                      int64_t n_items,
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
    const int64_t n_in = n_items * M; // samples
    const int hl = (Q - 1) * M + 1;   // virt()'s filter length: hl - 1 history samples
    const int64_t m0 = (int64_t)blockIdx.x * g::T;
    const int64_t g0 = (m0 - (Q - 1)) * M; // stream sample (of this call) at window position 0
    const int count = rows * M;

    float2 w[LOG2M > 1 ? LOG2M - 1 : 1];
#pragma unroll
    for (int s = 0; s < LOG2M - 1; ++s) w[s] = tw[s * M + p];
    const int wcol = col_entry<M>((int)(__builtin_bitreverse32((unsigned)p) >> (32 - LOG2M)));

    // Window positions [b, b + kBlock n): position i is channel i mod M of row i / M; kBlock is a
    // multiple of M, so a lane keeps its channel and the M lanes of a row are in or out together.
    auto stage = [&](auto load, int b, auto n) {
        constexpr int N = decltype(n)::value;
        if (b + 64 * wave >= count) return; // nothing of the pass for this wave (the halo's last pass)
        float2 a[N];
#pragma unroll
        for (int u = 0; u < N; ++u) {
            const int i = b + kBlock * u + tid;
            a[u] = i < count ? load(i) : make_float2(0.f, 0.f);
        }
        lane_dft<M, N>(a, w, p);
#pragma unroll
        for (int u = 0; u < N; ++u) {
            const int i = b + kBlock * u + tid;
            if (i < count) xs[g::row_entry(i >> LOG2M) + wcol] = a[u];
        }
    };
    auto stage_all = [&](auto load) {
        stage(load, 0, std::integral_constant<int, kStage>());
        for (int b = kBlock * kStage; b < count; b += kBlock * kTail) stage(load, b, std::integral_constant<int, kTail>());
    };
    if (g0 >= 0 && g0 + count <= n_in)
        stage_all([&](int i) { return ld_nt(in + g0 + i); });
    else
        stage_all([&](int i) { return virt(in, hist_in, g0 + i, n_in, hl); });
    for (int i = tid; i < Qp * M; i += kBlock) hs[i] = hp[i];
    if (blockIdx.x == 0) nsh::store_history<kBlock>(in, hist_in, hist_out, n_in, hl, tid);

    const int qv = (L - p + M - 1) >> LOG2M; // this branch's taps: q < qv
    const int qall = L >> LOG2M;             // taps every branch has: q < qall
    const int col = col_entry<M>(p);
    float2* yw = ys + wave * g::YW;
    __syncthreads();

    const int trow = tg * kR; // the lane's first item in the tile
    auto row = [&](int rho) { return xs[g::row_entry(trow + max(rho, 0)) + col]; };

    float2 acc[kR];
#pragma unroll
    for (int t = 0; t < kR; ++t) acc[t] = make_float2(0.f, 0.f);
    // tap q = q0 + dq of item t meets row t + Q-1 - q = lo + k, k = t + kQC-1 - dq
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

    // the wave's 64 R / M items start at mw; its time group tgl holds items tgl R + t
    const int tgl = lane >> LOG2M;
    const int64_t mw = m0 + wave * (64 / M) * kR;
#pragma unroll
    for (int rd = 0; rd < nsh::pfb::kRounds; ++rd) {
        wave_lds_sync(); // the reads of the round before
#pragma unroll
        for (int t = 0; t < g::RH; ++t) yw[g::ypos(((tgl * g::RH + t) << LOG2M) + p)] = acc[rd * g::RH + t];
        wave_lds_sync();
        // image entry e: time group e / (RH M), then RH items of M outputs
        if (vec) {
#pragma unroll
            for (int i = 0; i < g::RH / 2; ++i) {
                const int e = 2 * (64 * i + lane);
                const int blk = e >> (ilog2(g::RH) + LOG2M), rest = e & (g::RH * M - 1);
                const int64_t m = mw + blk * kR + rd * g::RH + (rest >> LOG2M);
                if (m < n_items) {
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
                if (m < n_items) {
                    const float2 a = yw[g::ypos(e)];
                    const nf2 v = { a.x, a.y };
                    __builtin_nontemporal_store(v, reinterpret_cast<nf2*>(out + m * M + (rest & (M - 1))));
                }
            }
        }
    }
}

struct synth_plan : nsh::stream_plan { // tile: items per workgroup T; buf: Qp M taps, then the twiddles
    int L = 0, M = 0, Q = 0, Qp = 0;
    // the instantiation's launcher (setup)
    void (*launch)(const synth_plan*, const float2*, const float2*, float2*, float2*, int64_t, int, unsigned,
                   hipStream_t) = nullptr;
};

template <int M>
void launch_synth(const synth_plan* p, const float2* in, const float2* hin, float2* hout, float2* out, int64_t n_items,
                  int vec, unsigned grid, hipStream_t s)
{
    nsh::launch((k_pfb_synth<M>), dim3(grid), dim3(kBlock), (uint32_t)p->lds, s, in, hin, hout, out, (const float*)p->buf,
                (const float2*)((const float*)p->buf + p->Qp * M), p->L, p->Q, p->Qp, n_items, vec);
}

template <int M>
void setup(synth_plan* p)
{
    using g = geom<M>;
    p->tile = g::T;
    p->fn = (const void*)k_pfb_synth<M>;
    p->launch = launch_synth<M>;
    p->lds = (size_t)g::row_entry(g::T + p->Q - 1) * sizeof(float2) + (size_t)p->Qp * M * sizeof(float) +
             (size_t)(kBlock / 64) * g::YW * sizeof(float2);
}

} // namespace

extern "C" {

int nsh_pfb_synth_plan_create(int dev, const float* taps_host, int ntaps, int nchans, void** plan)
{
    if (!taps_host || !plan) return nsh::fail_msg("nsh_pfb_synth_plan_create: null pointer");
    if (ntaps < 1 || ntaps > 1024) return nsh::fail_msg("nsh_pfb_synth_plan_create: ntaps must be in [1, 1024]");
    if (nchans < 2 || nchans > 64 || (nchans & (nchans - 1)))
        return nsh::fail_msg("nsh_pfb_synth_plan_create: nchans must be a power of two in [2, 64]");
    const int Q = (ntaps + nchans - 1) / nchans;
    if (Q > 32)
        return nsh::fail_msg("nsh_pfb_synth_plan_create: at most 32 taps per branch (ceil(ntaps / nchans) <= 32)");
    NSH_CK(hipSetDevice(dev));
    auto p = std::make_unique<synth_plan>();
    p->dev = dev;
    p->L = ntaps;
    p->hist = (Q - 1) * nchans;
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
    p->kernel = "k_pfb_synth<" + std::to_string(nchans) + ">";
    const int M = nchans;
    const size_t ntap = (size_t)p->Qp * M; // a multiple of 8 floats: the twiddles are 8-byte aligned
    std::vector<float> host(ntap + nsh::pfb::twiddle_floats(M), 0.f);
    for (int k = 0; k < ntaps; ++k) host[k] = taps_host[k]; // hp[q M + r] = h[r + q M]
    nsh::pfb::fill_twiddles(M, host.data() + ntap);
    if (const int rc = p->upload(host.data(), host.size() * sizeof(float), "nsh_pfb_synth_plan_create")) return rc;
    *plan = p.release();
    return 0;
}

int nsh_pfb_synth_plan_destroy(void* plan)
{
    delete static_cast<synth_plan*>(plan);
    return 0;
}

int nsh_pfb_synth_tile(void* plan) { return plan ? static_cast<synth_plan*>(plan)->tile : 0; }
const char* nsh_pfb_synth_kernel(void* plan) { return plan ? static_cast<synth_plan*>(plan)->kernel.c_str() : ""; }

int nsh_pfb_synthesizer_ccf(void* plan, const float* in, const float* hist_in, float* hist_out, float* out, int64_t n_in,
                            void* stream)
{
    nsh::launch_events_guard timing_guard; // the armed event pair never outlives this call
    auto* p = static_cast<synth_plan*>(plan);
    unsigned grid = 0;
    const int rc = nsh::check_stream_call("nsh_pfb_synthesizer_ccf", p, in, hist_in, hist_out, out, n_in, INT64_MAX / 128,
                                          "(ceil(ntaps/nchans)-1)*nchans", "items", &grid);
    if (rc || !grid) return rc;
    const int vec = nsh::store_vec16(out, p->tile * p->M);
    p->launch(p, (const float2*)in, (const float2*)hist_in, (float2*)hist_out, (float2*)out, n_in, vec, grid,
              nsh::S(stream));
    NSH_CK_LAUNCH("nsh_pfb_synthesizer_ccf");
    return 0;
}

} // extern "C"
