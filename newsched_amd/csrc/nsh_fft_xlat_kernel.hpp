// k_fft_xlat<N, D, ROT>: the kernel of freq_xlating_fft_filter_ccc (<N, D>) and of fft_filter_ccc
// (<N, 1, false>: O = L-1, inc = 0, the rotation and its step table compiled out). nsh_fft_ols.hip
// has the definitions, the frames and the entry points; nsh_fft_xlat_<N>.hip instantiate the forms
// of one N each (seven D and the one without rotation), so that the 32 forms compile side by side.
// gfx950 only.
//
// A team of geom<N>::TT = N/16 lanes (nsh_fft_team.hpp) holds one frame, 16 samples a lane:
//
//   window -> fft_team<N, false> -> times Hs -> image in natural order
//          -> fold to M = N/D bins -> inverse of M points -> drop O/D -> times phasor -> store
//
// D = 1 has nothing to fold: the lanes read the image back in in_idx order and run fft_team<N, true>.
//
// Hs lies in the order the lanes meet it after the forward transform (entry m TT + t is
// Hs[geom::out_idx(t, m)]), so a wave reads it as whole lines. A lane meets the same 16 entries in
// every frame: N <= 4096 keeps them in registers for the whole kernel, N = 8192 (512 lanes, 256
// VGPRs each) reads them from L2 after every forward transform.
//
// Windows start at any 8-byte aligned sample and overlap, so a frame gets a buffer resource of its
// own: base in + (fV-O), length what is left of the stream, at most N. What lies past the end reads
// zeros without an address being formed for it, and the loop issues the same loads for every frame:
// the next frame's stay in flight across this frame's arithmetic. Only frame 0 of a call has
// positions below 0 (V >= O); the team that owns it loads it before the loop, history and input
// through one resource each. Stores go through a resource over the frame's Vd outputs, clipped at
// out + n_out; the lanes below O/D get an offset no resource reaches.
//
// Fold (D > 1). Z[k'] = ((Y[k'] + Y[k'+M]) + Y[k'+2M]) + ... + Y[k'+(D-1)M], d ascending, by all
// lanes of the team: lane t sums bins k' = t + FL j, j < BPL = max(16/D, 1), over FL = M / BPL
// lanes (every lane to D = 16, M of the N/16 lanes at D = 32 and 64), 16 LDS reads a lane as in the
// reorder step it replaces (D reads at D > 16). The sums go back to image entries [0, M) after a
// barrier (every Y has been read), and a second barrier hands them to the inverse.
//
// Inverse of M points inside a team sized for N:
//   M <= 1024  wave 0 of the team runs fft_team<M, true> with geom<M> (64 lanes; for M < 1024 that
//              geometry packs 1024/M frames, of which frame 0 is Z and the others are zeros), wave
//              barriers only; the team's other waves wait at one workgroup barrier after it.
//   M >= 2048  (N = 4096 D = 2; N = 8192 D = 2, 4: the team is the workgroup) the waves below M/1024
//              run fft_team<M, true>, whose team_sync is the workgroup barrier; the others run the
//              same number of barriers (team_syncs(M)) and nothing else. The branch is on the wave
//              index read into an SGPR, so no wave walks both sides.
// The M-point passes take their twiddles from the N-point tables already in LDS: a pass's table
// depends on (Ns, R) alone (nsh_fft_team.hpp, NTAB).
// The inverse's lanes then hold z[i] = y[window position i D] at i = geom<M>::out_idx(t, m); those
// with O/D <= i < M are rotated and stored through a resource over the frame's Vd outputs clipped at
// out + n_out. The phase of output o = f Vd + i - O/D is ((first_index + o D) inc) mod 2^64; a lane
// takes one sincospif per frame, for its first output's phase, and multiplies it by
// steps[m] = phasor(c(m) D inc) from a 16-entry LDS table for output m, which lies c(m) outputs on
// (two phasors of 2^-32 turns of truncation each and one rounded complex product, in place of
// sixteen sincospif a lane). inc == 0 skips the rotation (a uniform branch); ROT = false has no
// branch, no table and no phasor code: with them fft_filter_ccc's launches took 2 to 3 % longer at
// N = 4096 and 8192 than the kernel without.
//
// Budgets, from the compiler's kernel-resource-usage remarks: LDS is the twiddle
// tables of N, one padded image per team and (ROT) the 128-byte step table, 42.0 / 50.0 / 66.0 /
// 132.0 KiB per workgroup at N = 1024 / 2048 / 4096 / 8192; 232 to 254 VGPRs (ROT = false: 220 to
// 238), no AGPRs, two waves per SIMD in all forms; no scratch and no VGPR spill in any. 15 of the
// 21 forms with D > 1 hold more
// scalars than there are SGPRs and keep 30 to 38 of them in VGPR lanes (SGPR spill in the remarks; no
// memory). The lane index is re-read through an empty asm before the fold (tq): with its addresses
// hoisted out of the frame loop next to the forward transform's, the D > 1 forms took 256 VGPRs and up
// to 71 AGPRs (one wave per SIMD) and N = 8192 spilled to scratch. DESIGN.md 4.10.
#pragma once
#include "nsh_fft_ols.hpp"
#include "nsh_phase.hpp"
#include "nsh_stream_tile.hpp"

namespace nsh {
namespace fxlat {

using nsh::cf;
using nsh::cmulw;
using nsh::fft::fft_team;
using nsh::fft::geom;
using nsh::fft::pad;
using nsh::fft::radix_at;
using nsh::fft::team_sync;
using nsh::ols::buf_load_cf;
using nsh::ols::kNowhere;
using nsh::ols::span_rsrc;

struct args {
    const float2* in;
    const float2* hist_in;
    float2* hist_out;
    float2* out;
    int64_t n_out;
    int L, O;
    uint64_t inc, first;
    const float2* tw;
    const float2* hs;
};
using launch_fn = void (*)(const args&, unsigned grid, hipStream_t s);
// the launcher of k_fft_xlat<N, D, rot>, D in {1, 2, 4, 8, 16, 32, 64}; rot = false (no rotation:
// the caller's inc is 0) exists at D = 1 only (nsh_fft_xlat_<N>.hip)
template <int N>
launch_fn launcher(int D, bool rot);
template <>
launch_fn launcher<1024>(int D, bool rot);
template <>
launch_fn launcher<2048>(int D, bool rot);
template <>
launch_fn launcher<4096>(int D, bool rot);
template <>
launch_fn launcher<8192>(int D, bool rot);

// team_sync calls of fft_team<n, INV>, n > 16
constexpr int team_syncs(int n)
{
    int c = 1;
    for (int ns = 16; ns < n; ns *= radix_at(n, ns)) c += ns * radix_at(n, ns) < n ? 2 : 1;
    return c;
}

template <int N>
constexpr bool hs_in_regs = geom<N>::NT <= 256;

template <int N, int D, bool ROT = true>
__global__ __launch_bounds__(geom<N>::NT) void k_fft_xlat(const float2* __restrict__ in, const float2* __restrict__ hist_in,
                                                          float2* __restrict__ hist_out, float2* __restrict__ out,
                                                          int64_t n_out, int L, int O, uint64_t inc, uint64_t first,
                                                          const float2* __restrict__ tw_g, const float2* __restrict__ hs_g)
{
    using G = geom<N>;
    constexpr int M = N / D;
    using GM = geom<M>;
    static_assert(G::F == 1 && M >= 16, "one frame per team, an inverse of at least 16 points");
    constexpr bool HREG = hs_in_regs<N>;
    constexpr bool ONE_WAVE = M <= 1024; // the inverse runs in the team's wave 0
    static_assert(D == 1 || ONE_WAVE || G::TEAMS == 1, "a sub-team of several waves meets at workgroup barriers");
    __shared__ cf tw[G::TWN];
    __shared__ cf img_all[G::TEAMS * G::IMG];
    // steps[m] = phasor(c(m) D inc), c(m) = TT (m % NBL) + QL (m / NBL) of geom<M>: output m of a lane
    // of the inverse sits c(m) outputs after the lane's first (store_frame)
    __shared__ float2 steps[16];
    nsh::fft::stage_table(tw, tw_g, G::TWN, threadIdx.x, G::NT);
    if constexpr (ROT) {
        if (threadIdx.x < 16) {
            const int m = threadIdx.x;
            steps[m] = nsh::phasor((uint64_t)(GM::TT * (m % GM::NBL) + GM::QL * (m / GM::NBL)) * ((uint64_t)D * inc));
        }
    }
    __syncthreads();
    const int t = threadIdx.x & (G::TT - 1), team = threadIdx.x / G::TT;
    // the wave's index in its team, in an SGPR
    const int tw_wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) & (G::TT / 64 - 1);
    cf* img = img_all + team * G::IMG;
    const int H = L - 1, V = N - O, Od = O / D, Vd = V / D;
    const int64_t n_in = n_out * D;
    const int64_t nframes = (n_out + Vd - 1) / Vd, ngroups = (nframes + G::TILE - 1) / G::TILE;

    // window of frame f >= 1 (V >= O: it starts at or after the call's first sample)
    const auto load_window = [&](cf(&v)[16], int64_t f) {
        const int64_t w0 = f * V - O;
        int64_t items = n_in - w0;
        items = items < 0 ? 0 : (items > N ? N : items);
        const __amdgpu_buffer_rsrc_t r = span_rsrc(in + (items > 0 ? w0 : 0), items);
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = buf_load_cf(r, G::in_idx(t, m) * 8);
    };
    // window of frame 0: O - H zeros, H samples of history (zeros without one), then the input
    const auto load_first = [&](cf(&v)[16]) {
        const __amdgpu_buffer_rsrc_t rh = span_rsrc(hist_in, hist_in ? H : 0);
        const __amdgpu_buffer_rsrc_t ri = span_rsrc(in, n_in < V ? n_in : V);
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const int p = G::in_idx(t, m);
            const cf a = buf_load_cf(rh, p < O && p >= O - H ? (p - (O - H)) * 8 : kNowhere);
            const cf b = buf_load_cf(ri, p >= O ? (p - O) * 8 : kNowhere);
            v[m] = p < O ? a : b;
        }
    };
    // the inverse's lanes: z[i] at i = GM::out_idx(t, m), rotated, to out[f Vd + i - Od]
    const auto store_frame = [&](const cf(&v)[16], int64_t f, int t) {
        const int64_t o0 = f * Vd;
        int64_t items = n_out - o0;
        items = items < 0 ? 0 : (items > Vd ? Vd : items);
        const __amdgpu_buffer_rsrc_t r = span_rsrc(out + (items > 0 ? o0 : 0), items);
        if (!ROT || inc == 0) {
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const int i = GM::out_idx(t, m);
                nsh::buf_store_f2(r, i >= Od && i < M ? (i - Od) * 8 : kNowhere, v[m]);
            }
        } else {
            // A lane's outputs of frame 0 sit at i = t + c(m), c(m) = TT (m % NBL) + QL (m / NBL) (out_idx
            // where it is below M). One sincospif a lane and frame, for the lane's own phase; output m
            // takes it times steps[m], one rounded complex product more (k_fir_xlat's pair trick).
            // With sixteen sincospif a lane the kernel took 297 us instead of 229 per 2^26 inputs at
            // D = 1 and 266 instead of 208 at D = 8 (127 taps).
            const uint64_t pstep = (uint64_t)D * inc;
            const float2 w0 = nsh::phasor((first + (uint64_t)o0 * (uint64_t)D) * inc + (uint64_t)(int64_t)(t - Od) * pstep);
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const int i = GM::out_idx(t, m);
                const float2 y = nsh::crot(make_float2(v[m].x, v[m].y), nsh::crot(w0, steps[m]));
                nsh::buf_store_f2(r, i >= Od && i < M ? (i - Od) * 8 : kNowhere, nsh::buf_f2{ y.x, y.y });
            }
        }
    };

    int64_t g = blockIdx.x;
    if (g >= ngroups) return;
    cf hs[16];
    if constexpr (HREG) {
#pragma unroll
        for (int m = 0; m < 16; ++m) hs[m] = cf{ hs_g[m * G::TT + t].x, hs_g[m * G::TT + t].y };
    }
    // every team of the workgroup walks the same number of steps (workgroup barriers inside): a team
    // past the last frame loads zeros and its stores are dropped
    cf v[16], nx[16];
    if (g * G::TEAMS + team == 0)
        load_first(v);
    else
        load_window(v, g * G::TEAMS + team);
    for (; g < ngroups; g += gridDim.x) {
        const int64_t f = g * G::TEAMS + team;
        load_window(nx, f + (int64_t)gridDim.x * G::TEAMS);
        fft_team<N, false>(v, img, tw, t);
        if constexpr (!HREG) {
#pragma unroll
            for (int m = 0; m < 16; ++m) hs[m] = cf{ hs_g[m * G::TT + t].x, hs_g[m * G::TT + t].y };
        }
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = cmulw(v[m], hs[m]);
        // the spectrum lies as the forward transform left it; the image takes it in natural order
#pragma unroll
        for (int m = 0; m < 16; ++m) img[pad(G::out_idx(t, m))] = v[m];
        team_sync<G::WG>();
        if constexpr (D == 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = img[pad(G::in_idx(t, r))];
            team_sync<G::WG>();
            fft_team<N, true>(v, img, tw, t);
            store_frame(v, f, t);
        } else {
            constexpr int BPL = D <= 16 ? 16 / D : 1, FL = M / BPL;
            // the lane index again, opaque to the compiler: the fold's and the M-point transform's LDS
            // addresses are then formed in every frame instead of living in 40 to 70 registers across
            // the loop, next to the forward transform's own
            int tq = t;
            asm volatile("" : "+v"(tq));
            cf z[BPL];
            if (FL >= G::TT || tq < FL) {
#pragma unroll
                for (int j = 0; j < BPL; ++j) {
                    const int k = tq + FL * j;
                    cf s = img[pad(k)];
#pragma unroll
                    for (int d = 1; d < D; ++d) s = s + img[pad(k + d * M)];
                    z[j] = s;
                }
            }
            team_sync<G::WG>(); // every Y has been read
            if (FL >= G::TT || tq < FL) {
#pragma unroll
                for (int j = 0; j < BPL; ++j) img[pad(tq + FL * j)] = z[j];
            }
            team_sync<G::WG>();
            if constexpr (ONE_WAVE) {
                if (tw_wave == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int p = GM::in_idx(tq, r);
                        v[r] = p < M ? img[pad(p < M ? p : 0)] : cf{ 0.f, 0.f };
                    }
                    team_sync<false>();
                    fft_team<M, true, N>(v, img, tw, tq);
                    store_frame(v, f, tq);
                }
                if constexpr (G::WG) team_sync<true>(); // the image is free for the next frame
            } else {
                const bool sub = tw_wave < M / 1024;
                if (sub) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) v[r] = img[pad(GM::in_idx(tq, r))];
                }
                team_sync<true>();
                if (sub) {
                    fft_team<M, true, N>(v, img, tw, tq);
                    store_frame(v, f, tq);
                } else {
                    for (int i = 0; i < team_syncs(M); ++i) team_sync<true>();
                }
            }
        }
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = nx[m];
    }
    if (blockIdx.x == 0) nsh::store_history<G::NT>(in, hist_in, hist_out, n_in, L, threadIdx.x);
}

template <int N, int D, bool ROT = true>
void launch_form(const args& a, unsigned grid, hipStream_t s)
{
    nsh::launch((k_fft_xlat<N, D, ROT>), dim3(grid), dim3(geom<N>::NT), 0, s, a.in, a.hist_in, a.hist_out, a.out, a.n_out, a.L, a.O,
                a.inc, a.first, a.tw, a.hs);
}

// the body of launcher<N>, for the one file that instantiates N's forms
#define NSH_FFT_XLAT_FORMS(N)                                                                                                  \
    template <>                                                                                                                \
    nsh::fxlat::launch_fn nsh::fxlat::launcher<N>(int D, bool rot)                                                             \
    {                                                                                                                          \
        if (!rot) return D == 1 ? launch_form<N, 1, false> : nullptr;                                                          \
        switch (D) {                                                                                                           \
        case 1: return launch_form<N, 1>;                                                                                      \
        case 2: return launch_form<N, 2>;                                                                                      \
        case 4: return launch_form<N, 4>;                                                                                      \
        case 8: return launch_form<N, 8>;                                                                                      \
        case 16: return launch_form<N, 16>;                                                                                    \
        case 32: return launch_form<N, 32>;                                                                                    \
        case 64: return launch_form<N, 64>;                                                                                    \
        default: return nullptr;                                                                                               \
        }                                                                                                                      \
    }

} // namespace fxlat
} // namespace nsh
