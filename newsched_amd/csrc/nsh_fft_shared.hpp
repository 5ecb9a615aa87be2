// The pieces every FFT kernel of libnsh_hip.so is built from (k_fft1024 and k_chan1024 in
// nsh_fft.hip, k_fft<N> in nsh_fft_plan.hip, k_fft_xlat<N, D> in nsh_fft_xlat_kernel.hpp; the last two
// share the team transform of nsh_fft_team.hpp on top of this file): the register DFT16, the padded LDS image, the
// conjugation switch, twiddle staging and the 16-samples-per-lane buffer loads and stores.
// gfx950 only.
#pragma once
#include "nsh_common.hpp"
#include "nsh_cplx.hpp"

#include <cmath>
#include <vector>

namespace nsh {
namespace fft {

// W_16^m, m = 0..9 (forward; conjugated for the inverse)
template <bool INV>
__device__ __forceinline__ cf w16(int m)
{
    constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508978f, R2 = 0.70710678118654757f;
    cf w;
    switch (m) {
    case 1: w = cf{ C1, -S1 }; break;
    case 2: w = cf{ R2, -R2 }; break;
    case 3: w = cf{ S1, -C1 }; break;
    case 4: w = cf{ 0.f, -1.f }; break;
    case 6: w = cf{ -R2, -R2 }; break;
    case 9: w = cf{ -C1, S1 }; break;
    default: w = cf{ 1.f, 0.f }; break;
    }
    if (INV) w.y = -w.y;
    return w;
}

// In-place DFT16, natural order in and out: n = 4 n1 + n2, k = k1 + 4 k2,
// X[k] = sum_n2 W_4^{n2 k2} W_16^{n2 k1} sum_n1 x[4 n1 + n2] W_4^{n1 k1}.
template <bool INV>
__device__ __forceinline__ void dft16(cf (&v)[16])
{
#pragma unroll
    for (int n2 = 0; n2 < 4; ++n2) dft4<INV>(v[n2], v[n2 + 4], v[n2 + 8], v[n2 + 12]); // v[n2 + 4 k1] = Y[n2][k1]
#pragma unroll
    for (int n2 = 1; n2 < 4; ++n2)
#pragma unroll
        for (int k1 = 1; k1 < 4; ++k1) {
            const int m = n2 * k1;
            if (m == 4) // W_16^4 = -+i
                v[n2 + 4 * k1] = rot<INV>(v[n2 + 4 * k1]);
            else
                v[n2 + 4 * k1] = cmulw(v[n2 + 4 * k1], w16<INV>(m));
        }
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) dft4<INV>(v[4 * k1], v[4 * k1 + 1], v[4 * k1 + 2], v[4 * k1 + 3]); // v[4 k1 + k2] = X[k1 + 4 k2]
    cf t[16];
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1)
#pragma unroll
        for (int k2 = 0; k2 < 4; ++k2) t[k1 + 4 * k2] = v[4 * k1 + k2];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = t[k];
}

// LDS image index: one pad sample per 16, so the passes' strided exchanges spread over the banks
__device__ __forceinline__ int pad(int i) { return i + (i >> 4); }
constexpr int padded(int n) { return n + n / 16; }

template <bool INV>
__device__ __forceinline__ cf conj_if(cf w)
{
    if (INV) w.y = -w.y;
    return w;
}

// a workgroup's copy of n table entries (twiddles, weights) from global memory into LDS
__device__ __forceinline__ void stage_table(cf* __restrict__ t, const float2* __restrict__ g, int n, int tid, int nt)
{
    for (int i = tid; i < n; i += nt) t[i] = cf{ g[i].x, g[i].y };
}

// e^{-2 pi i e / n} rounded once from double: every table entry of every size (host)
inline float2 twiddle(int e, int n)
{
    const double a = -2.0 * M_PI * (double)e / (double)n;
    return make_float2((float)std::cos(a), (float)std::sin(a));
}

// A lane's 16 samples of chunk ch of a stream of n samples (chunks of CH), sample idx(m) of the chunk
// into / from v[m], by buffer loads / stores over that chunk alone: what lies past the end of the
// stream reads zeros and drops its stores, so a loop issues the same memory instructions every
// iteration (no conditional prefetch) and the compiler's vmcnt waits stay exact -- the next
// chunk's loads remain in flight across this chunk's transform and stores.
template <int CH, typename Idx>
__device__ __forceinline__ void load16(cf (&v)[16], const float2* __restrict__ in, int64_t ch, int64_t n, Idx idx)
{
    const __amdgpu_buffer_rsrc_t r = chunk_rsrc<CH>(in, ch, n);
#pragma unroll
    for (int m = 0; m < 16; ++m)
        v[m] = __builtin_bit_cast(cf, __builtin_amdgcn_raw_buffer_load_b64(r, idx(m) * 8, 0, AUX_LD));
}
template <int CH, typename Idx>
__device__ __forceinline__ void store16(const cf (&v)[16], float2* __restrict__ out, int64_t ch, int64_t n, Idx idx)
{
    const __amdgpu_buffer_rsrc_t r = chunk_rsrc<CH>(out, ch, n);
#pragma unroll
    for (int m = 0; m < 16; ++m) buf_store_f2(r, idx(m) * 8, v[m]);
}
// sample j + 64 m: a wave's coalesced walk over a 1024-sample chunk
struct lane64 {
    int j;
    __device__ __forceinline__ int operator()(int m) const { return j + 64 * m; }
};

// a plan's host table to a fresh allocation on the current device; nothing for an empty one
template <typename T>
int to_device(const std::vector<T>& h, T** dst)
{
    if (h.empty()) return 0;
    NSH_CK(hipMalloc(dst, h.size() * sizeof(T)));
    NSH_CK(hipMemcpy(*dst, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// Workgroups of a grid-stride walk over groups of fw frames, at most cap
inline unsigned frame_grid(int64_t nframes, int fw, int64_t cap)
{
    const int64_t groups = (nframes + fw - 1) / fw;
    return (unsigned)(groups < cap ? groups : cap);
}

// k_fft1024 (nsh_fft.hip) over nframes frames with at most cap workgroups (0: its default); takes
// the armed timing pair. The plan entry point's N = 1024 plain case and nsh_fft1024_c2c.
int fft1024_launch(const float2* in, float2* out, int64_t nframes, bool inverse, int cap, hipStream_t s, const char* what);

} // namespace fft
} // namespace nsh
