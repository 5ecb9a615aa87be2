// The team transform of the plan-based FFT kernels: k_fft<N> (nsh_fft_plan.hip) and
// k_fft_xlat<N, D> (nsh_fft_xlat_kernel.hpp). nsh_fft_plan.hip's header comment has the organisation (Stockham autosort,
// 16 samples per lane, teams of TT lanes, radix plan, per-pass twiddle tables); this file holds its
// geometry, the passes, fft_team and the host's table builder. gfx950 only.
#pragma once
#include "nsh_fft_shared.hpp"

#include <vector>

namespace nsh {
namespace fft {

constexpr int radix_at(int n, int ns) { return n / ns >= 16 ? 16 : n / ns; }
// entries of all per-pass twiddle tables of size n
constexpr int tw_count(int n)
{
    int c = 0;
    for (int ns = 16; ns < n; ns *= radix_at(n, ns)) c += (radix_at(n, ns) - 1) * ns;
    return c;
}
constexpr int last_radix(int n)
{
    int r = 16;
    for (int ns = 16; ns < n; ns *= r) r = radix_at(n, ns);
    return r;
}

template <int N>
struct geom {
    static constexpr int TT = N / 16 > 64 ? N / 16 : 64; // lanes of a team
    static constexpr int S = 16 * TT;                    // samples of a team
    static constexpr int F = S / N;                      // frames of a team
    static constexpr int NT = TT > 256 ? TT : 256;       // workgroup
    static constexpr int TEAMS = NT / TT;
    static constexpr int TILE = TEAMS * F;               // frames per workgroup
    static constexpr int IMG = nsh::fft::padded(S);      // a team's LDS image
    static constexpr bool WG = TT > 64;                  // teams of several waves: workgroup barriers
    static constexpr int TWN = tw_count(N);
    static constexpr int RL = last_radix(N), NBL = 16 / RL, QL = N / RL;
    // chunk index of the sample pass 1 takes into register r, and of the one the last pass
    // leaves in register m = i + NBL r (the host orders tables by them too)
    __host__ __device__ static __forceinline__ int in_idx(int t, int r)
    {
        return (t / (N / 16)) * N + (t & (N / 16 - 1)) + (N / 16) * r;
    }
    __host__ __device__ static __forceinline__ int out_idx(int t, int m)
    {
        const int b = t + TT * (m % NBL);
        return (b / QL) * N + (b & (QL - 1)) + QL * (m / NBL);
    }
};

template <bool WG>
__device__ __forceinline__ void team_sync()
{
    if (WG)
        nsh::lds_barrier();
    else
        __builtin_amdgcn_wave_barrier(); // a wave's LDS operations complete in order
}

template <int R, bool INV>
__device__ __forceinline__ void dft_r(cf (&a)[R])
{
    if constexpr (R == 16)
        dft16<INV>(a);
    else if constexpr (R == 8)
        dft8<INV>(a);
    else if constexpr (R == 4)
        dft4<INV>(a[0], a[1], a[2], a[3]);
    else {
        const cf s = a[0] + a[1], d = a[0] - a[1];
        a[0] = s;
        a[1] = d;
    }
}

// pass (Ns, R) of the team: image -> twiddles -> butterflies -> v[i + NB r]. TWK > 1: tw is the
// pass's table of a larger size whose radix here is TWK R (W_{Ns R}^{kr} = W_{Ns TWK R}^{k TWK r}).
template <int N, int Ns, int R, bool INV, int TWK = 1>
__device__ __forceinline__ void pass_read(cf (&v)[16], const cf* __restrict__ img, const cf* __restrict__ tw, int t)
{
    constexpr int NB = 16 / R, Q = N / R, TT = geom<N>::TT;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int b = t + TT * i, j = b & (Q - 1), k = j & (Ns - 1), base = (b / Q) * N + j;
        cf a[R];
#pragma unroll
        for (int r = 0; r < R; ++r) a[r] = img[pad(base + Q * r)];
#pragma unroll
        for (int r = 1; r < R; ++r) a[r] = cmulw(a[r], conj_if<INV>(tw[(r * TWK - 1) * Ns + k]));
        dft_r<R, INV>(a);
#pragma unroll
        for (int r = 0; r < R; ++r) v[i + NB * r] = a[r];
    }
}
// ... and v[i + NB r] -> image, autosorted
template <int N, int Ns, int R>
__device__ __forceinline__ void pass_write(const cf (&v)[16], cf* __restrict__ img, int t)
{
    constexpr int NB = 16 / R, Q = N / R, TT = geom<N>::TT;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int b = t + TT * i, j = b & (Q - 1), k = j & (Ns - 1), base = (b / Q) * N + (j - k) * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r) img[pad(base + Ns * r)] = v[i + NB * r];
    }
}

// the passes from sub-transform size Ns on; the image holds pass input. The last pass's output
// stays in v (geom::out_idx). tw holds the tables of size NTAB >= N (pass_tables(NTAB)): a pass's
// table depends on (Ns, R) alone, so a smaller transform walks a prefix of a larger one's.
template <int N, int Ns, bool INV, int NTAB = N>
__device__ __forceinline__ void passes_from(cf (&v)[16], cf* __restrict__ img, const cf* __restrict__ tw, int t)
{
    constexpr int R = radix_at(N, Ns);
    constexpr bool WG = geom<N>::WG;
    pass_read<N, Ns, R, INV, radix_at(NTAB, Ns) / R>(v, img, tw, t);
    team_sync<WG>(); // all reads done before the image is rewritten (by the next pass or the next tile)
    if constexpr (Ns * R < N) {
        pass_write<N, Ns, R>(v, img, t);
        team_sync<WG>();
        passes_from<N, Ns * R, INV, NTAB>(v, img, tw + (R - 1) * Ns, t);
    }
}

// Transform of the team's frames held as v[r] = x[geom::in_idx(t, r)]; on return v[m] =
// X[geom::out_idx(t, m)].
template <int N, bool INV, int NTAB = N>
__device__ __forceinline__ void fft_team(cf (&v)[16], cf* __restrict__ img, const cf* __restrict__ tw, int t)
{
    dft16<INV>(v);
    if constexpr (N > 16) {
        pass_write<N, 1, 16>(v, img, t);
        team_sync<geom<N>::WG>();
        passes_from<N, 16, INV, NTAB>(v, img, tw, t);
    }
}

// T[r - 1][k] = W_{Ns R}^{k r} of every pass after the first, concatenated; each entry is
// e^{-2 pi i e / n} of the reduced exponent e < n, as in k_fft1024's table
inline std::vector<float2> pass_tables(int n)
{
    std::vector<float2> h;
    for (int ns = 16; ns < n; ns *= radix_at(n, ns)) {
        const int R = radix_at(n, ns), m = n / (ns * R);
        for (int r = 1; r < R; ++r)
            for (int k = 0; k < ns; ++k) h.push_back(twiddle((m * k * r) & (n - 1), n));
    }
    return h;
}

} // namespace fft
} // namespace nsh
