// Host arithmetic of pfb_arb_resampler_ccf (include/nsh_hip.h, the pfb_arb_resampler section): the
// Q32.32 step of a rate and the span of a call -- how many outputs n_in inputs hold from a phase, how
// many inputs they consume and the phase handed to the next call. Exact integer arithmetic, no HIP:
// libnsh_hip.so (nsh_arb_step, nsh_arb_span, the check of nsh_arb_resamp_ccf) and both blocks
// (blocks::pfb_arb_resampler_ccf, hip::pfb_arb_resampler_ccf) use this one copy.
//
//   step     = round(F / r * 2^32), filter steps per output (F = nfilt filters per input sample)
//   pos(n)   = phase + n * step: the position of output n relative to in[0], exact and unbounded
//   k(n)     = pos(n) >> 32, input i(n) = k(n) div F, filter j(n) = k(n) mod F,
//   mu(n)    = float((pos(n) & 0xffffffff) >> 8) * 2^-24
#pragma once
#include <cmath>
#include <cstdint>

namespace nsh_arb {

constexpr int64_t kMaxItems = 0x7fffffff; // n_in and n_out of one call

// log2 of nfilt when it is a power of two in [2, 64], else -1
inline int filt_shift(int nfilt)
{
    for (int s = 1; s <= 6; ++s)
        if (nfilt == (1 << s)) return s;
    return -1;
}

inline bool rate_ok(double rate) { return std::isfinite(rate) && rate >= 1.0 / 64 && rate <= 64.0; }

// round(nfilt * 2^32 / rate), exact from the double (ties to even), for a rate_ok rate and a
// filt_shift-ed nfilt: at most 2^44, at least 2^27.
inline uint64_t step_of(double rate, int nfilt)
{
    const double N = std::ldexp((double)nfilt, 32);
    double s = std::nearbyint(N / rate); // within one of the exact answer
    // N - s rate is a multiple of rate's last bit and smaller than rate: the fma gives it exactly
    const double e = std::fma(-s, rate, N), half = 0.5 * rate;
    const bool odd = std::fmod(s, 2.0) != 0;
    if (e > half || (e == half && odd))
        s += 1;
    else if (e < -half || (e == -half && odd))
        s -= 1;
    return (uint64_t)s;
}

// a step that step_of can return for this nfilt
inline bool step_ok(uint64_t step, int fshift) { return step >= (1ull << (26 + fshift)) && step <= (1ull << (38 + fshift)); }

struct span {
    int64_t n_out;       // outputs of the call: min(want, what n_in inputs hold from phase)
    int64_t n_consumed;  // c = min(i(n_out), n_in)
    uint64_t phase_next; // pos(n_out) - c F 2^32
};

// 0 <= n_in, want <= kMaxItems, step_ok(step, fshift). The outputs n with i(n) <= n_in - 1 are those
// with pos(n) < n_in F 2^32: ceil((n_in F 2^32 - phase) / step) of them when that is positive.
inline span span_of(uint64_t step, int fshift, uint64_t phase, int64_t n_in, int64_t want)
{
    typedef unsigned __int128 u128;
    const u128 end = (u128)(uint64_t)n_in << (32 + fshift);
    int64_t n_max = 0;
    if (end > phase) {
        const u128 m = (end - phase + step - 1) / step;
        n_max = m > (u128)kMaxItems ? kMaxItems : (int64_t)m;
    }
    span r;
    r.n_out = want < n_max ? want : n_max;
    const u128 pos = (u128)phase + (u128)(uint64_t)r.n_out * step;
    const u128 i = pos >> (32 + fshift);
    r.n_consumed = i < (u128)(uint64_t)n_in ? (int64_t)i : n_in;
    r.phase_next = (uint64_t)(pos - ((u128)(uint64_t)r.n_consumed << (32 + fshift)));
    return r;
}

// fl32(h[k+1] - h[k]), 0 for the last tap: GNU Radio's create_diff_taps
inline void diff_taps(const float* h, int ntaps, float* d)
{
    for (int k = 0; k + 1 < ntaps; ++k) {
        volatile float v = h[k + 1] - h[k];
        d[k] = v;
    }
    d[ntaps - 1] = 0.f;
}

} // namespace nsh_arb
