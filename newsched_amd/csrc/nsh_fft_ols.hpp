// What the overlap-save kernel k_fft_xlat<N, D> (nsh_fft_xlat_kernel.hpp) and its plan
// (nsh_fft_ols.hip) are built from. Per-window buffer resources on the device; the taps' spectrum,
// the default frame size and the default grid cap on the host. gfx950 only.
// The times below were measured on k_fft_filter<N>, which k_fft_xlat<N, 1, false> replaced (same sequence).
#pragma once
#include "nsh_fft_team.hpp"

#include <cmath>
#include <vector>

namespace nsh {
namespace ols {

// items samples (8 B each) from base on; built from wave-uniform values only (chunk_rsrc)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t span_rsrc(const float2* base, int64_t items)
{
    const uint64_t a = (uint64_t)base;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    const int bytes = __builtin_amdgcn_readfirstlane((int)(items * 8));
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), (short)0, bytes, 0x00020000);
}
// a byte offset past every resource of these kernels (at most 64 KiB), far from wrapping
constexpr int kNowhere = 0x40000000;

__device__ __forceinline__ cf buf_load_cf(__amdgpu_buffer_rsrc_t r, int byte_off)
{
    return __builtin_bit_cast(cf, __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, 0, nsh::AUX_LD));
}

// (1/N) DFT_N of the zero-padded taps ((re, im) pairs of T = float or double), in double, rounded
// once (1/N is a power of two: exact)
template <typename T>
std::vector<float2> spectrum_of(const T* taps, int L, int N)
{
    std::vector<double> wr(N), wi(N);
    for (int j = 0; j < N; ++j) {
        const double a = -2.0 * M_PI * (double)j / (double)N;
        wr[j] = std::cos(a);
        wi[j] = std::sin(a);
    }
    std::vector<float2> s(N);
    for (int k = 0; k < N; ++k) {
        double re = 0.0, im = 0.0;
        for (int i = 0; i < L; ++i) {
            const double hr = taps[2 * i], hi = taps[2 * i + 1];
            if (hr == 0.0 && hi == 0.0) continue;
            const int e = (int)(((int64_t)k * i) & (N - 1));
            re += hr * wr[e] - hi * wi[e];
            im += hr * wi[e] + hi * wr[e];
        }
        s[k] = make_float2((float)(re / N), (float)(im / N));
    }
    return s;
}

// Default frame size: the smallest N >= 4 pow2ceil(L) up to 4096, the smallest N >= 2 pow2ceil(L)
// beyond, at least 1024: 1024 to 256 taps, 2048 to 512, 4096 to 2048, 8192 above. The candidates
// were rule2 (N >= 2 pow2ceil(L)) and rule4 (N >= 4 pow2ceil(L)): fewer, longer frames overlap less,
// and a frame of 8192 costs 1.5 times one of 4096 per sample (512 lanes, one workgroup per CU, the
// spectrum re-read). Kernel times of fft_filter_ccc on 2^26 samples, rule2 / rule4
// (tools/fft_filter_bench.py, profiles/fft_filter_bench.json): 512 taps 345 / 345 us,
// 1024 taps 462 / 340 us, 2048 taps 457 / 546 us; to 256 and above 2048 taps the two rules give the
// same size.
inline int default_fft_size(int L)
{
    int p = 1;
    while (p < L) p *= 2;
    const int n = 4 * p <= 4096 ? 4 * p : 2 * p;
    return n < 1024 ? 1024 : n;
}

// Workgroups of the grid-stride walk. A workgroup stages its size's twiddle tables once and
// prefetches from its second step on; fft_filter_ccc, 127 taps on 2^26 samples under caps of
// 256 .. 16384 (tools/fft_filter_bench.py --cap-sweep), us at 256 / 512 / 1024 / 2048 /
// 8192 workgroups: N = 1024: 266 / 222 / 220 / 217 / 244, 2048: 341 / 255 / 254 / 253 / 273,
// 4096: 315 / 253 / 251 / 254 / 270, 8192: 385 / 387 / 392 / 401 / 479. 512 to 2048 are level up to
// 4096 points (within the rounds' spread), 256 and 512 at 8192.
constexpr int default_cap(int n) { return n <= 4096 ? 1024 : 512; }

} // namespace ols
} // namespace nsh
