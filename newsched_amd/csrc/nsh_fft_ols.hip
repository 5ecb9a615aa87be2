// libnsh_hip.so: the overlap-save filters, one plan and one kernel family for both.
//
// freq_xlating_fft_filter_ccc: tune, filter with complex taps and decimate in one launch.
//
//   y[m] = sum_{k<L} h[k] x[mD-k] exp(+j 2 pi phase(first_index + mD - k))
//        = exp(+j 2 pi phase(first_index + mD)) sum_{k<L} g[k] x[mD-k],
//   g[k] = h[k] exp(-j 2 pi ((k inc) mod 2^64) / 2^64),   phase(n) = ((n inc) mod 2^64) / 2^64 turns,
//
// x, h complex fp32, 1 <= L <= 4096, D in {1, 2, 4, 8, 16, 32, 64}, inc = nsh_phase_inc(-freq_norm)
// (nsh_xlat.hip has the phase). The second line is what runs: the band-pass taps g are formed in
// double on the host from the 64-bit inc the kernel uses, their spectrum Hs = (1/N) DFT_N(g) is
// rounded once (ols::spectrum_of), and the rotation that is left meets the 1/D outputs on their way
// out, phasor((first_index + m D) inc) in uint64 wrap-around: an output's phase does not depend on
// how the stream is cut. inc == 0 skips the rotation.
//
// fft_filter_ccc, y[n] = sum_{k<L} h[k] x[n-k], is the case D = 1, inc = 0 (g = h exactly, O = L-1,
// first_index 0) of the same plan and the same kernel, in the form without the rotation
// (k_fft_xlat<N, 1, false>).
//
// Frames of N in {1024, 2048, 4096, 8192} samples, L <= N/2; O = L-1 rounded up to a multiple of D
// (O <= N/2), V = N - O, Vd = V/D outputs a frame, M = N/D >= 16. Frame f owns out[f Vd, (f+1) Vd)
// up to n_out and reads the window x[fV-O, fV-O+N) of the call's n_out D inputs: history (or
// zeros) in [-(L-1), 0), zeros below (they reach discarded outputs only) and at or past n_out D.
// nsh_fft_xlat_kernel.hpp has the kernel: forward transform, times Hs, fold to M bins, inverse of M
// points, drop O/D, rotate, store.
#include "nsh_fft_xlat_kernel.hpp"

#include <cmath>
#include <memory>
#include <string>
#include <vector>

namespace {

using nsh::fft::geom;
using nsh::fxlat::launch_fn;

struct ols_plan {
    int dev = 0, n = 0, L = 0, D = 0, O = 0, tile = 0, cap = 0, cap_default = 0;
    uint64_t inc = 0;
    float2* tw = nullptr;
    float2* hs = nullptr;
    std::string kernel;
    launch_fn launch = nullptr;
    std::vector<float2> tw_host, hs_host; // until they are on the device
    ~ols_plan()
    {
        nsh::dev_free(tw);
        nsh::dev_free(hs);
    }
    // the twiddle tables and Hs to the current device
    int upload()
    {
        if (const int rc = nsh::fft::to_device(tw_host, &tw)) return rc;
        if (const int rc = nsh::fft::to_device(hs_host, &hs)) return rc;
        tw_host = std::vector<float2>();
        hs_host = std::vector<float2>();
        return 0;
    }
};

int refuse(const char* who, const char* why) { return nsh::fail_msg((std::string(who) + ": " + why).c_str()); }

// Hs in the lanes' order: entry m TT + t = Hs[out_idx(t, m)]
template <int N>
void setup(ols_plan* p, const std::vector<float2>& spectrum, bool rot)
{
    using G = geom<N>;
    p->tile = G::TILE;
    p->launch = nsh::fxlat::launcher<N>(p->D, rot);
    p->hs_host.resize(N);
    for (int m = 0; m < 16; ++m)
        for (int t = 0; t < G::TT; ++t) p->hs_host[m * G::TT + t] = spectrum[G::out_idx(t, m)];
}

// g[k] = h[k] exp(-j 2 pi ((k inc) mod 2^64) / 2^64) in double; the phase as a signed fraction of a
// turn (the short way round). inc == 0: g = h exactly.
std::vector<double> bandpass_taps(const float* taps, int L, uint64_t inc)
{
    std::vector<double> g(2 * (size_t)L);
    for (int k = 0; k < L; ++k) {
        const double hr = taps[2 * k], hi = taps[2 * k + 1];
        if (inc == 0) {
            g[2 * k] = hr, g[2 * k + 1] = hi;
            continue;
        }
        const double th = -2.0 * M_PI * std::ldexp((double)(int64_t)((uint64_t)k * inc), -64);
        const double c = std::cos(th), s = std::sin(th);
        g[2 * k] = hr * c - hi * s;
        g[2 * k + 1] = hr * s + hi * c;
    }
    return g;
}

// The plan of either entry point (who names it in the refusals), tables on the host: no HIP call.
// nsh_fft_filter_plan_create passes decim 1 and freq_norm 0, which the two checks it does not have
// let through, and rot = false: the kernel form without the rotation.
int make_plan(const char* who, int dev, const float* taps_host, int ntaps, int decim, double freq_norm, bool rot, int fft_size,
              void** plan, std::unique_ptr<ols_plan>& made)
{
    if (!taps_host || !plan) return refuse(who, "null pointer");
    if (ntaps < 1 || ntaps > 4096) return refuse(who, "ntaps must be in [1, 4096]");
    for (int i = 0; i < 2 * ntaps; ++i)
        if (!std::isfinite(taps_host[i])) return refuse(who, "tap is not finite");
    if (decim < 1 || decim > 64 || (decim & (decim - 1))) return refuse(who, "decimation must be a power of two in [1, 64]");
    uint64_t inc = 0;
    if (!std::isfinite(freq_norm) || nsh_phase_inc(-freq_norm, &inc)) return refuse(who, "the frequency must be finite");
    if (fft_size != 0 && fft_size != 1024 && fft_size != 2048 && fft_size != 4096 && fft_size != 8192)
        return refuse(who, "fft_size must be 0, 1024, 2048, 4096 or 8192");
    if (fft_size && ntaps > fft_size / 2) return refuse(who, "ntaps must be at most fft_size / 2");
    // frame size and grid cap: the rules of nsh_fft_ols.hpp, which were measured at D = 1, inc = 0;
    // tools/fft_xlat_bench.py --rules and --cap-sweep measure them for the other forms
    const int N = fft_size ? fft_size : nsh::ols::default_fft_size(ntaps);
    auto p = std::make_unique<ols_plan>();
    p->dev = dev;
    p->n = N;
    p->L = ntaps;
    p->D = decim;
    p->O = (ntaps - 1 + decim - 1) / decim * decim;
    p->inc = inc;
    p->cap_default = p->cap = nsh::ols::default_cap(N);
    p->kernel = "k_fft_xlat<" + std::to_string(N) + ", " + std::to_string(decim) + (rot ? ">" : ", false>");
    const std::vector<double> g = bandpass_taps(taps_host, ntaps, inc);
    const std::vector<float2> spectrum = nsh::ols::spectrum_of(g.data(), ntaps, N);
    switch (N) {
    case 1024: setup<1024>(p.get(), spectrum, rot); break;
    case 2048: setup<2048>(p.get(), spectrum, rot); break;
    case 4096: setup<4096>(p.get(), spectrum, rot); break;
    default: setup<8192>(p.get(), spectrum, rot); break;
    }
    p->tw_host = nsh::fft::pass_tables(N);
    made = std::move(p);
    return 0;
}

int grid_cap(const char* who, void* plan, int max_workgroups)
{
    if (max_workgroups < 0) return refuse(who, "negative cap");
    if (!plan) return refuse(who, "null plan");
    auto* p = static_cast<ols_plan*>(plan);
    p->cap = max_workgroups ? max_workgroups : p->cap_default;
    return 0;
}

int run(const char* who, void* plan, const float* in, const float* hist_in, float* hist_out, float* out, int64_t n_out,
        uint64_t first_index, void* stream)
{
    nsh::launch_events_guard timing_guard; // an armed event pair never outlives this call
    if (n_out <= 0) return 0;
    if (!in || !out) return refuse(who, "null input or output");
    if (in == out) return refuse(who, "in-place not supported");
    if (hist_in && hist_in == hist_out) return refuse(who, "hist_out must not alias hist_in");
    if (!plan) return refuse(who, "null plan");
    auto* p = static_cast<ols_plan*>(plan);
    if (!hist_out && p->L > 1) return refuse(who, "hist_out is required (ntaps-1 samples)");
    if (n_out > INT64_MAX / 16 / p->D) return refuse(who, "too many samples for one call");
    if (!p->tw) // a plan made where there was no device
        if (const int rc = p->upload()) return rc;
    const int Vd = (p->n - p->O) / p->D;
    const int64_t nframes = (n_out + Vd - 1) / Vd;
    nsh::fxlat::args a;
    a.in = (const float2*)in, a.hist_in = (const float2*)hist_in, a.hist_out = (float2*)hist_out, a.out = (float2*)out;
    a.n_out = n_out, a.L = p->L, a.O = p->O, a.inc = p->inc, a.first = first_index;
    a.tw = p->tw, a.hs = p->hs;
    p->launch(a, nsh::fft::frame_grid(nframes, p->tile, p->cap), nsh::S(stream));
    NSH_CK_LAUNCH(who);
    return 0;
}

const ols_plan* P(void* plan) { return static_cast<const ols_plan*>(plan); }

} // namespace

extern "C" {

int nsh_fft_filter_plan_create(int dev, const float* taps_host, int ntaps, int fft_size, void** plan)
{
    std::unique_ptr<ols_plan> p;
    if (const int rc = make_plan("nsh_fft_filter_plan_create", dev, taps_host, ntaps, 1, 0.0, false, fft_size, plan, p))
        return rc;
    NSH_CK(hipSetDevice(dev));
    if (const int rc = p->upload()) return rc;
    *plan = p.release();
    return 0;
}

int nsh_fft_xlat_plan_create(int dev, const float* taps_host, int ntaps, int decim, double freq_norm, int fft_size, void** plan)
{
    std::unique_ptr<ols_plan> p;
    if (const int rc = make_plan("nsh_fft_xlat_plan_create", dev, taps_host, ntaps, decim, freq_norm, true, fft_size, plan, p))
        return rc;
    // On a machine without any device the plan is still made (its geometry can be asked for); its
    // tables then go up with the first nsh_fft_xlat_ccc, which fails there if there is still none.
    const hipError_t e = hipSetDevice(dev);
    if (e == hipErrorNoDevice)
        (void)hipGetLastError();
    else if (e != hipSuccess)
        return nsh::fail(e, "hipSetDevice(dev)");
    else if (const int rc = p->upload())
        return rc;
    *plan = p.release();
    return 0;
}

int nsh_fft_filter_plan_destroy(void* plan)
{
    delete static_cast<ols_plan*>(plan);
    return 0;
}
int nsh_fft_xlat_plan_destroy(void* plan) { return nsh_fft_filter_plan_destroy(plan); }

int nsh_fft_xlat_fft_size(void* plan) { return plan ? P(plan)->n : 0; }
int nsh_fft_xlat_decim(void* plan) { return plan ? P(plan)->D : 0; }
int nsh_fft_xlat_overlap(void* plan) { return plan ? P(plan)->O : 0; }
int nsh_fft_xlat_valid(void* plan) { return plan ? P(plan)->n - P(plan)->O : 0; }
int nsh_fft_xlat_history(void* plan) { return plan ? P(plan)->L - 1 : 0; }
int nsh_fft_xlat_phase_inc(void* plan, uint64_t* inc)
{
    if (!plan || !inc) return nsh::fail_msg("nsh_fft_xlat_phase_inc: null pointer");
    *inc = P(plan)->inc;
    return 0;
}
int nsh_fft_xlat_tile(void* plan) { return plan ? P(plan)->tile : 0; }
const char* nsh_fft_xlat_kernel(void* plan) { return plan ? P(plan)->kernel.c_str() : ""; }

// a filter plan has D = 1: O = L - 1
int nsh_fft_filter_fft_size(void* plan) { return nsh_fft_xlat_fft_size(plan); }
int nsh_fft_filter_valid(void* plan) { return nsh_fft_xlat_valid(plan); }
int nsh_fft_filter_history(void* plan) { return nsh_fft_xlat_history(plan); }
int nsh_fft_filter_tile(void* plan) { return nsh_fft_xlat_tile(plan); }
const char* nsh_fft_filter_kernel(void* plan) { return nsh_fft_xlat_kernel(plan); }

int nsh_fft_filter_grid_cap(void* plan, int max_workgroups) { return grid_cap("nsh_fft_filter_grid_cap", plan, max_workgroups); }
int nsh_fft_xlat_grid_cap(void* plan, int max_workgroups) { return grid_cap("nsh_fft_xlat_grid_cap", plan, max_workgroups); }

int nsh_fft_filter_ccc(void* plan, const float* in, const float* hist_in, float* hist_out, float* out, int64_t n, void* stream)
{
    return run("nsh_fft_filter_ccc", plan, in, hist_in, hist_out, out, n, 0, stream);
}

int nsh_fft_xlat_ccc(void* plan, const float* in, const float* hist_in, float* hist_out, float* out, int64_t n_out,
                     uint64_t first_index, void* stream)
{
    return run("nsh_fft_xlat_ccc", plan, in, hist_in, hist_out, out, n_out, first_index, stream);
}

} // extern "C"
