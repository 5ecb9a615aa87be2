// CPU block implementations (reference blocklib/blocks/lib/*.cpp semantics).
#include <gnuradio/blocklib/blocks/arith.hpp>
#include <gnuradio/blocklib/blocks/fft.hpp>
#include <gnuradio/blocklib/blocks/fft_filter.hpp>
#include <gnuradio/blocklib/blocks/fir_filter_ccf.hpp>
#include <gnuradio/blocklib/blocks/freq_xlating_fft_filter_ccc.hpp>
#include <gnuradio/blocklib/blocks/freq_xlating_fir_filter_ccf.hpp>
#include <gnuradio/blocklib/blocks/pfb_arb_resampler_ccf.hpp>
#include <gnuradio/blocklib/blocks/pfb_channelizer_ccf.hpp>
#include <gnuradio/blocklib/blocks/pfb_synthesizer_ccf.hpp>
#include <gnuradio/blocklib/blocks/psd.hpp>
#include <gnuradio/blocklib/blocks/rational_resampler_ccf.hpp>
#include <gnuradio/blocklib/blocks/multiply_const.hpp>
#include <gnuradio/blocklib/blocks/rotator_cc.hpp>

#include "../../csrc/nsh_arb_span.hpp"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <stdexcept>

namespace gr {
namespace blocks {

namespace {
// Function multiversioning by ISA FEATURE. GCC's target_clones("arch=skylake-avx512", "arch=haswell",
// "default") -- what this file used up to round 5 -- dispatches "arch=" clones with
// __builtin_cpu_is(<model>), which is false on every AMD EPYC and on Intel parts GCC does not name
// that way (this container's Xeon included), so the baseline ran the SSE2 default clone. The clones
// below are chosen with __builtin_cpu_supports on the features each one is compiled for.
enum class isa { avx512, avx2, base };
isa detect_isa()
{
    __builtin_cpu_init();
    if (__builtin_cpu_supports("avx512f") && __builtin_cpu_supports("fma")) return isa::avx512;
    if (__builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma")) return isa::avx2;
    return isa::base;
}
const isa g_isa = detect_isa();
#define NSR_AVX512 __attribute__((target("avx512f,avx512vl,avx512dq,avx512bw,avx2,fma")))
#define NSR_AVX2 __attribute__((target("avx2,fma")))

// (ar kr - ai ki, ar ki + ai kr) with every product rounded: FMA contraction is switched
// off for these two functions only, to match the reference formula bit for bit.
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
static inline __attribute__((always_inline)) void cmul_const_body(const float* in, float* out, size_t n, float kr, float ki)
{
    for (size_t i = 0; i < n; ++i) {
        const float ar = in[2 * i], ai = in[2 * i + 1];
        const float p0 = ar * kr, p1 = ai * ki, p2 = ar * ki, p3 = ai * kr;
        out[2 * i] = p0 - p1;
        out[2 * i + 1] = p2 + p3;
    }
}
static inline __attribute__((always_inline)) void cmul_vec_body(const float* a, const float* b, float* out, size_t n)
{
    for (size_t i = 0; i < n; ++i) {
        const float ar = a[2 * i], ai = a[2 * i + 1], br = b[2 * i], bi = b[2 * i + 1];
        const float p0 = ar * br, p1 = ai * bi, p2 = ar * bi, p3 = ai * br;
        out[2 * i] = p0 - p1;
        out[2 * i + 1] = p2 + p3;
    }
}
NSR_AVX512 void cmul_const_avx512(const float* in, float* out, size_t n, float kr, float ki) { cmul_const_body(in, out, n, kr, ki); }
NSR_AVX2 void cmul_const_avx2(const float* in, float* out, size_t n, float kr, float ki) { cmul_const_body(in, out, n, kr, ki); }
void cmul_const_base(const float* in, float* out, size_t n, float kr, float ki) { cmul_const_body(in, out, n, kr, ki); }
NSR_AVX512 void cmul_vec_avx512(const float* a, const float* b, float* out, size_t n) { cmul_vec_body(a, b, out, n); }
NSR_AVX2 void cmul_vec_avx2(const float* a, const float* b, float* out, size_t n) { cmul_vec_body(a, b, out, n); }
void cmul_vec_base(const float* a, const float* b, float* out, size_t n) { cmul_vec_body(a, b, out, n); }
#pragma GCC pop_options

void cmul_const(const float* in, float* out, size_t n, float kr, float ki)
{
    switch (g_isa) {
    case isa::avx512: return cmul_const_avx512(in, out, n, kr, ki);
    case isa::avx2: return cmul_const_avx2(in, out, n, kr, ki);
    default: return cmul_const_base(in, out, n, kr, ki);
    }
}
void cmul_vec(const float* a, const float* b, float* out, size_t n)
{
    switch (g_isa) {
    case isa::avx512: return cmul_vec_avx512(a, b, out, n);
    case isa::avx2: return cmul_vec_avx2(a, b, out, n);
    default: return cmul_vec_base(a, b, out, n);
    }
}

// Decim-1 rows: NV x 8 complex outputs (NV vectors of 16 interleaved floats) per step, fp32
// accumulation: out[m] = sum_k h[k] * x[m - k], x = ext shifted by L-1. The taps go by residue
// rho = k mod 8: tap rho + 8t at output vector r reads the input vector W[r - t] (one vector = 8
// complex samples = the 8-tap stride), so for one residue each input vector is loaded ONCE, aligned
// to the 8-sample grid of its residue, and feeds up to NV FMAs from a rolling window of NV
// registers -- instead of one cache-line-splitting load per FMA. NV = 8 on AVX-512 (two FMA
// pipes x four cycles of latency), 4 on AVX2 (the same registers in 256-bit halves).
typedef float v16f __attribute__((vector_size(64)));

template <int NV, int P>
static inline __attribute__((always_inline)) void fir_step(v16f* a, v16f* w, float hk)
{
    for (int r = 0; r < NV; ++r) a[r] += hk * w[(r - P + 8 * NV) % NV];
}

template <int NV>
static inline __attribute__((always_inline)) void fir_rows_body(const float* ext, const float* h, int L, int D, float* out,
                                                                size_t n_out)
{
    size_t m = 0;
    if (D == 1) {
        for (; m + 8 * NV <= n_out; m += 8 * NV) {
            v16f a[NV] = {};
            const float* base = ext + 2 * (m + (size_t)(L - 1));
            for (int rho = 0; rho < 8 && rho < L; ++rho) {
                const float* W = base - 2 * rho; // W[j] = W + 16 j
                const int T = (L - rho + 7) / 8;  // taps rho, rho + 8, ... < L
                v16f w[NV];                       // W[j] in slot j mod NV
                for (int r = 0; r < NV; ++r) std::memcpy(&w[r], W + 16 * r, 64);
                // step t: a[r] += h[rho + 8t] W[r - t]; then W[-(t+1)] replaces W[NV-1-t]
#define NSR_FIR_STEP(P)                                                                      \
    if (t + P < T) {                                                                         \
        fir_step<NV, P % NV>(a, w, h[rho + 8 * (t + P)]);                                    \
        if (t + P + 1 < T) std::memcpy(&w[(NV - 1 - P % NV) % NV], W - 16 * (t + P + 1), 64); \
    }
                for (int t = 0; t < T; t += 8) {
                    NSR_FIR_STEP(0) NSR_FIR_STEP(1) NSR_FIR_STEP(2) NSR_FIR_STEP(3)
                    NSR_FIR_STEP(4) NSR_FIR_STEP(5) NSR_FIR_STEP(6) NSR_FIR_STEP(7)
                }
#undef NSR_FIR_STEP
            }
            for (int r = 0; r < NV; ++r) std::memcpy(out + 2 * m + 16 * r, &a[r], 64);
        }
    }
    for (; m < n_out; ++m) {
        float ar = 0.f, ai = 0.f;
        for (int k = 0; k < L; ++k) {
            const float* x = ext + 2 * (m * (size_t)D + (size_t)(L - 1 - k));
            ar += h[k] * x[0];
            ai += h[k] * x[1];
        }
        out[2 * m] = ar;
        out[2 * m + 1] = ai;
    }
}
NSR_AVX512 void fir_rows_avx512(const float* ext, const float* h, int L, int D, float* out, size_t n)
{
    fir_rows_body<8>(ext, h, L, D, out, n);
}
NSR_AVX2 void fir_rows_avx2(const float* ext, const float* h, int L, int D, float* out, size_t n)
{
    fir_rows_body<4>(ext, h, L, D, out, n);
}
void fir_rows_base(const float* ext, const float* h, int L, int D, float* out, size_t n) { fir_rows_body<4>(ext, h, L, D, out, n); }
void fir_rows(const float* ext, const float* h, int L, int D, float* out, size_t n_out)
{
    switch (g_isa) {
    case isa::avx512: return fir_rows_avx512(ext, h, L, D, out, n_out);
    case isa::avx2: return fir_rows_avx2(ext, h, L, D, out, n_out);
    default: return fir_rows_base(ext, h, L, D, out, n_out);
    }
}
} // namespace

template <class T>
work_return_code_t multiply_const<T>::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const T* iptr = static_cast<const T*>(in[0].buffer->read_ptr());
    T* optr = static_cast<T*>(out[0].buffer->write_ptr());
    const size_t n = (size_t)out[0].n_items * d_vlen;
    if constexpr (std::is_same_v<T, gr_complex>) {
        cmul_const(reinterpret_cast<const float*>(iptr), reinterpret_cast<float*>(optr), n, d_k.real(), d_k.imag());
    } else {
        for (size_t i = 0; i < n; ++i) optr[i] = iptr[i] * d_k;
    }
    out[0].n_produced = out[0].n_items;
    return work_return_code_t::WORK_OK;
}
template class multiply_const<int16_t>;
template class multiply_const<int32_t>;
template class multiply_const<float>;
template class multiply_const<gr_complex>;

template <int OP>
work_return_code_t arith_cc<OP>::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const size_t n = (size_t)out[0].n_items * _vlen;
    float* o = static_cast<float*>(out[0].buffer->write_ptr());
    const float* a = static_cast<const float*>(in[0].buffer->read_ptr());
    if (_nports == 1) {
        if (o != a) std::memmove(o, a, n * 8);
    }
    for (size_t p = 1; p < _nports; ++p) {
        const float* b = static_cast<const float*>(in[p].buffer->read_ptr());
        const float* src = p == 1 ? a : o;
        if constexpr (OP == 0) {
            for (size_t i = 0; i < 2 * n; ++i) o[i] = src[i] + b[i];
        } else {
            cmul_vec(src, b, o, n);
        }
    }
    out[0].n_produced = out[0].n_items;
    return work_return_code_t::WORK_OK;
}
template class arith_cc<0>;
template class arith_cc<1>;

fir_filter_ccf::fir_filter_ccf(const std::vector<float>& taps, int decim)
    : decim_block("fir_filter_ccf", (unsigned)decim), _taps(taps), _decim(decim)
{
    if (taps.empty()) throw std::invalid_argument("fir_filter_ccf: no taps");
    if (decim < 1) throw std::invalid_argument("fir_filter_ccf: decimation < 1");
}

bool fir_filter_ccf::start()
{
    _ext.assign(_taps.size() - 1, gr_complex(0, 0)); // zero history at stream start
    return block::start();
}

void fir_filter_ccf::filter(const gr_complex* x, gr_complex* y, int n_out)
{
    const int L = (int)_taps.size();
    const size_t n_in = (size_t)n_out * _decim;
    if (_ext.size() < (size_t)(L - 1)) _ext.assign((size_t)(L - 1), gr_complex(0, 0)); // not started: zeros
    _ext.resize((size_t)(L - 1) + n_in);
    std::memcpy(_ext.data() + (L - 1), x, n_in * sizeof(gr_complex));
    fir_rows(reinterpret_cast<const float*>(_ext.data()), _taps.data(), L, _decim, reinterpret_cast<float*>(y), (size_t)n_out);
    // keep the last L-1 inputs as history
    std::memmove(_ext.data(), _ext.data() + n_in, (size_t)(L - 1) * sizeof(gr_complex));
    _ext.resize((size_t)(L - 1));
}

work_return_code_t fir_filter_ccf::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int n_out = out[0].n_items; // decim_block::do_work: in[0].n_items == D * n_out
    filter(static_cast<const gr_complex*>(in[0].buffer->read_ptr()), static_cast<gr_complex*>(out[0].buffer->write_ptr()),
           n_out);
    out[0].n_produced = n_out;
    return work_return_code_t::WORK_OK;
}

// ---- rotator_cc / freq_xlating_fir_filter_ccf: the 64-bit phase, double sincos -----------------
bool rotator_cc::start()
{
    _index = _first;
    return block::start();
}

work_return_code_t rotator_cc::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const gr_complex* x = static_cast<const gr_complex*>(in[0].buffer->read_ptr());
    gr_complex* y = static_cast<gr_complex*>(out[0].buffer->write_ptr());
    const int n = out[0].n_items;
    for (int i = 0; i < n; ++i) {
        double s, c;
        phase_sincos((_index + (uint64_t)i) * _inc, s, c);
        const double re = x[i].real(), im = x[i].imag();
        y[i] = gr_complex((float)(re * c - im * s), (float)(re * s + im * c));
    }
    _index += (uint64_t)n;
    out[0].n_produced = n;
    return work_return_code_t::WORK_OK;
}

freq_xlating_fir_filter_ccf::freq_xlating_fir_filter_ccf(int decim, const std::vector<float>& taps, double center_freq,
                                                         double samp_rate)
    : decim_block("freq_xlating_fir_filter_ccf", (unsigned)(decim > 0 ? decim : 1)), _taps(taps), _decim(decim)
{
    if (taps.empty()) throw std::invalid_argument("freq_xlating_fir_filter_ccf: no taps");
    if (decim < 1) throw std::invalid_argument("freq_xlating_fir_filter_ccf: decimation < 1");
    if (!(samp_rate > 0)) throw std::invalid_argument("freq_xlating_fir_filter_ccf: samp_rate must be positive");
    _inc = phase_inc_turns(-(center_freq / samp_rate));
}

bool freq_xlating_fir_filter_ccf::start()
{
    _ext.assign(_taps.size() - 1, gr_complex(0, 0)); // zero history at stream start
    _index = _first;
    return block::start();
}

work_return_code_t freq_xlating_fir_filter_ccf::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int n_out = out[0].n_items; // decim_block::do_work: in[0].n_items == D * n_out
    const int L = (int)_taps.size();
    const size_t n_in = (size_t)n_out * _decim;
    const gr_complex* x = static_cast<const gr_complex*>(in[0].buffer->read_ptr());
    gr_complex* y = static_cast<gr_complex*>(out[0].buffer->write_ptr());
    _ext.resize((size_t)(L - 1) + n_in);
    std::memcpy(_ext.data() + (L - 1), x, n_in * sizeof(gr_complex));
    // rotate every sample of the window once (the raw history is rotated again with its own phase)
    std::vector<std::complex<double>> rot(_ext.size());
    for (size_t i = 0; i < _ext.size(); ++i) {
        double s, c;
        phase_sincos((_index + (uint64_t)i - (uint64_t)(L - 1)) * _inc, s, c);
        const double re = _ext[i].real(), im = _ext[i].imag();
        rot[i] = std::complex<double>(re * c - im * s, re * s + im * c);
    }
    for (int m = 0; m < n_out; ++m) {
        std::complex<double> acc = 0;
        const std::complex<double>* w = rot.data() + (size_t)m * _decim + (L - 1);
        for (int k = 0; k < L; ++k) acc += (double)_taps[k] * w[-k];
        y[m] = gr_complex((float)acc.real(), (float)acc.imag());
    }
    std::memmove(_ext.data(), _ext.data() + n_in, (size_t)(L - 1) * sizeof(gr_complex)); // the last L-1 raw inputs
    _ext.resize((size_t)(L - 1));
    _index += (uint64_t)n_in;
    out[0].n_produced = n_out;
    return work_return_code_t::WORK_OK;
}

// ---- pfb_channelizer_ccf: straight from the definition, fp32 ---------------------------------------
pfb_channelizer_ccf::pfb_channelizer_ccf(int nchans, const std::vector<float>& taps)
    : decim_block("pfb_channelizer_ccf", (unsigned)(nchans > 0 ? nchans : 1)), _taps(taps), _nchans(nchans)
{
    if (taps.empty()) throw std::invalid_argument("pfb_channelizer_ccf: no taps");
    if (nchans < 2 || nchans > 64 || (nchans & (nchans - 1)))
        throw std::invalid_argument("pfb_channelizer_ccf: nchans must be a power of two in [2, 64]");
    _w.resize((size_t)nchans);
    for (int i = 0; i < nchans; ++i) {
        const double th = 2.0 * M_PI * (double)i / (double)nchans;
        _w[i] = gr_complex((float)std::cos(th), (float)std::sin(th));
    }
    // the quadrant points exactly
    _w[0] = gr_complex(1, 0);
    _w[nchans / 2] = gr_complex(-1, 0);
    if (nchans >= 4) _w[nchans / 4] = gr_complex(0, 1), _w[3 * nchans / 4] = gr_complex(0, -1);
}

bool pfb_channelizer_ccf::start()
{
    _ext.assign(_taps.size() - 1, gr_complex(0, 0)); // zero history at stream start
    return block::start();
}

work_return_code_t pfb_channelizer_ccf::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int n_out = out[0].n_items; // decim_block::do_work: in[0].n_items == M * n_out
    const int L = (int)_taps.size(), M = _nchans;
    const size_t n_in = (size_t)n_out * M;
    const gr_complex* x = static_cast<const gr_complex*>(in[0].buffer->read_ptr());
    gr_complex* y = static_cast<gr_complex*>(out[0].buffer->write_ptr());
    _ext.resize((size_t)(L - 1) + n_in);
    std::memcpy(_ext.data() + (L - 1), x, n_in * sizeof(gr_complex));
    for (int m = 0; m < n_out; ++m) {
        const gr_complex* w = _ext.data() + (size_t)m * M + (L - 1); // x[mM]
        for (int c = 0; c < M; ++c) {
            float re = 0.f, im = 0.f;
            for (int k = 0; k < L; ++k) {
                const gr_complex e = _w[(size_t)((c * k) & (M - 1))];
                const float hr = _taps[k] * e.real(), hi = _taps[k] * e.imag();
                const float xr = w[-k].real(), xi = w[-k].imag();
                re += hr * xr - hi * xi;
                im += hr * xi + hi * xr;
            }
            y[(size_t)m * M + c] = gr_complex(re, im);
        }
    }
    std::memmove(_ext.data(), _ext.data() + n_in, (size_t)(L - 1) * sizeof(gr_complex)); // the last L-1 raw inputs
    _ext.resize((size_t)(L - 1));
    out[0].n_produced = n_out;
    return work_return_code_t::WORK_OK;
}

// ---- pfb_synthesizer_ccf: polyphase form, fp32 ------------------------------------------------------
pfb_synthesizer_ccf::pfb_synthesizer_ccf(int nchans, const std::vector<float>& taps)
    : resamp_block("pfb_synthesizer_ccf", (unsigned)(nchans > 0 ? nchans : 1), 1), _taps(taps), _nchans(nchans)
{
    if (taps.empty()) throw std::invalid_argument("pfb_synthesizer_ccf: no taps");
    if (nchans < 2 || nchans > 64 || (nchans & (nchans - 1)))
        throw std::invalid_argument("pfb_synthesizer_ccf: nchans must be a power of two in [2, 64]");
    _w.resize((size_t)nchans);
    for (int i = 0; i < nchans; ++i) {
        const double th = 2.0 * M_PI * (double)i / (double)nchans;
        _w[i] = gr_complex((float)std::cos(th), (float)std::sin(th));
    }
    // the quadrant points exactly
    _w[0] = gr_complex(1, 0);
    _w[nchans / 2] = gr_complex(-1, 0);
    if (nchans >= 4) _w[nchans / 4] = gr_complex(0, 1), _w[3 * nchans / 4] = gr_complex(0, -1);
}

bool pfb_synthesizer_ccf::start()
{
    const size_t M = (size_t)_nchans, Q = (_taps.size() + M - 1) / M;
    _ext.assign((Q - 1) * M, gr_complex(0, 0)); // zero history at stream start
    return block::start();
}

work_return_code_t pfb_synthesizer_ccf::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int M = _nchans, L = (int)_taps.size(), Q = (L + M - 1) / M;
    const int n_in = out[0].n_items / M; // resamp_block::do_work: n items in, n M samples out
    const size_t H = (size_t)(Q - 1) * M, n_samp = (size_t)n_in * M;
    const gr_complex* x = static_cast<const gr_complex*>(in[0].buffer->read_ptr());
    gr_complex* y = static_cast<gr_complex*>(out[0].buffer->write_ptr());
    _ext.resize(H + n_samp);
    std::memcpy(_ext.data() + H, x, n_samp * sizeof(gr_complex));
    // v_r[m] = sum_c X[m][c] exp(j 2 pi c r / M), for the history's items too
    _v.resize(_ext.size());
    for (size_t j = 0; j < (size_t)(Q - 1 + n_in); ++j) {
        const gr_complex* X = _ext.data() + j * M;
        for (int r = 0; r < M; ++r) {
            float re = 0.f, im = 0.f;
            for (int c = 0; c < M; ++c) {
                const gr_complex e = _w[(size_t)((c * r) & (M - 1))];
                re += X[c].real() * e.real() - X[c].imag() * e.imag();
                im += X[c].real() * e.imag() + X[c].imag() * e.real();
            }
            _v[j * M + r] = gr_complex(re, im);
        }
    }
    for (int m = 0; m < n_in; ++m)
        for (int r = 0; r < M; ++r) {
            const gr_complex* v = _v.data() + ((size_t)(m + Q - 1)) * M + r; // v_r[m]
            float re = 0.f, im = 0.f;
            for (int k = r, q = 0; k < L; k += M, ++q) { // the taps that meet an item, none beyond L
                re += _taps[k] * v[-(ptrdiff_t)q * M].real();
                im += _taps[k] * v[-(ptrdiff_t)q * M].imag();
            }
            y[(size_t)m * M + r] = gr_complex(re, im);
        }
    std::memmove(_ext.data(), _ext.data() + n_samp, H * sizeof(gr_complex)); // the last Q-1 raw items
    _ext.resize(H);
    out[0].n_produced = n_in * M;
    return work_return_code_t::WORK_OK;
}

// ---- fft_vcc: radix-2 in double, rounded once ------------------------------------------------------
fft_vcc::fft_vcc(size_t fft_size, bool forward, const std::vector<float>& window, bool shift)
    : sync_block(forward ? "fft_vcc" : "ifft_vcc"), _fft_size(fft_size), _forward(forward), _shift(shift), _window(window)
{
    if (fft_size < 16 || fft_size > 8192 || (fft_size & (fft_size - 1)))
        throw std::invalid_argument("fft_vcc: fft_size must be a power of two in [16, 8192]");
    if (!window.empty() && window.size() != fft_size) throw std::invalid_argument("fft_vcc: the window must have fft_size entries");
    _tw.resize(fft_size / 2);
    for (size_t t = 0; t < fft_size / 2; ++t) {
        const double a = (forward ? -2.0 : 2.0) * M_PI * (double)t / (double)fft_size;
        _tw[t] = { std::cos(a), std::sin(a) };
    }
    _a.resize(fft_size);
}

work_return_code_t fft_vcc::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const size_t N = _fft_size, H = N / 2;
    const gr_complex* x = static_cast<const gr_complex*>(in[0].buffer->read_ptr());
    gr_complex* y = static_cast<gr_complex*>(out[0].buffer->write_ptr());
    size_t bits = 0;
    while (((size_t)1 << bits) < N) ++bits;
    for (int f = 0; f < out[0].n_items; ++f, x += N, y += N) {
        // window (fp32 products), the inverse's input shift and the bit reversal, in one placement
        for (size_t n = 0; n < N; ++n) {
            const size_t src = !_forward && _shift ? n ^ H : n;
            const float w = _window.empty() ? 1.f : _window[src];
            size_t rev = 0;
            for (size_t b = 0; b < bits; ++b) rev |= ((n >> b) & 1) << (bits - 1 - b);
            _a[rev] = { (double)(x[src].real() * w), (double)(x[src].imag() * w) };
        }
        for (size_t len = 2; len <= N; len <<= 1)
            for (size_t i = 0; i < N; i += len)
                for (size_t k = 0; k < len / 2; ++k) {
                    const std::complex<double> u = _a[i + k], v = _a[i + k + len / 2] * _tw[k * (N / len)];
                    _a[i + k] = u + v;
                    _a[i + k + len / 2] = u - v;
                }
        for (size_t k = 0; k < N; ++k) {
            const std::complex<double> v = _a[_forward && _shift ? k ^ H : k];
            y[k] = gr_complex((float)v.real(), (float)v.imag());
        }
    }
    out[0].n_produced = out[0].n_items;
    return work_return_code_t::WORK_OK;
}

// ---- rational_resampler_ccf: straight from the definition, fp32 -------------------------------------
rational_resampler_ccf::rational_resampler_ccf(int interp, int decim, const std::vector<float>& taps)
    : resamp_block("rational_resampler_ccf", (unsigned)(interp > 0 ? interp : 1), (unsigned)(decim > 0 ? decim : 1)),
      _taps(taps),
      _interp(interp),
      _decim(decim)
{
    if (taps.empty() || taps.size() > 1024) throw std::invalid_argument("rational_resampler_ccf: ntaps must be in [1, 1024]");
    if (interp < 1 || interp > 64) throw std::invalid_argument("rational_resampler_ccf: interpolation must be in [1, 64]");
    if (decim < 1 || decim > 64) throw std::invalid_argument("rational_resampler_ccf: decimation must be in [1, 64]");
}

bool rational_resampler_ccf::start()
{
    _ext.assign((_taps.size() + (size_t)_interp - 1) / (size_t)_interp - 1, gr_complex(0, 0)); // zero history
    return block::start();
}

work_return_code_t rational_resampler_ccf::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int I = _interp, D = _decim, L = (int)_taps.size();
    const int n_units = out[0].n_items / I; // resamp_block::do_work: n D inputs, n I outputs
    const size_t H = (size_t)((L + I - 1) / I - 1), n_in = (size_t)n_units * D;
    const gr_complex* x = static_cast<const gr_complex*>(in[0].buffer->read_ptr());
    gr_complex* y = static_cast<gr_complex*>(out[0].buffer->write_ptr());
    _ext.resize(H + n_in);
    std::memcpy(_ext.data() + H, x, n_in * sizeof(gr_complex));
    for (int n = 0; n < n_units * I; ++n) {
        const int phi = (int)(((int64_t)n * D) % I);
        const gr_complex* w = _ext.data() + H + (size_t)(((int64_t)n * D) / I); // x[j0]
        float re = 0.f, im = 0.f;
        for (int k = phi, q = 0; k < L; k += I, ++q) { // the taps that meet a sample, none beyond L
            re += _taps[k] * w[-q].real();
            im += _taps[k] * w[-q].imag();
        }
        y[n] = gr_complex(re, im);
    }
    std::memmove(_ext.data(), _ext.data() + n_in, H * sizeof(gr_complex)); // the last Q-1 raw inputs
    _ext.resize(H);
    out[0].n_produced = n_units * I;
    return work_return_code_t::WORK_OK;
}

// ---- pfb_arb_resampler_ccf: straight from the definition, fp32, exact integer phase ----------------
pfb_arb_resampler_ccf::pfb_arb_resampler_ccf(double rate, const std::vector<float>& taps, unsigned filter_size)
    : block("pfb_arb_resampler_ccf"), _rate(rate), _taps(taps), _nfilt(filter_size)
{
    _fshift = filter_size <= 64 ? nsh_arb::filt_shift((int)filter_size) : -1;
    if (_fshift < 0) throw std::invalid_argument("pfb_arb_resampler_ccf: nfilt must be a power of two in [2, 64]");
    if (taps.empty() || taps.size() > 2048) throw std::invalid_argument("pfb_arb_resampler_ccf: ntaps must be in [1, 2048]");
    if (!nsh_arb::rate_ok(rate)) throw std::invalid_argument("pfb_arb_resampler_ccf: rate must be finite and in [1/64, 64]");
    _step = nsh_arb::step_of(rate, (int)filter_size);
    _diff.resize(taps.size());
    nsh_arb::diff_taps(_taps.data(), (int)_taps.size(), _diff.data());
}

bool pfb_arb_resampler_ccf::start()
{
    const size_t H = (_taps.size() + _nfilt - 1) / _nfilt - 1;
    if (!_hist0.empty() && _hist0.size() != H)
        throw std::runtime_error("pfb_arb_resampler_ccf: the initial history must hold ceil(ntaps / nfilt) - 1 samples");
    _ext.assign(H, gr_complex(0, 0)); // zero history unless a shard's halo was given
    if (!_hist0.empty()) _ext = _hist0;
    _phase = _phase0;
    return block::start();
}

work_return_code_t pfb_arb_resampler_ccf::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int L = (int)_taps.size(), F = (int)_nfilt;
    const size_t H = (size_t)((L + F - 1) / F - 1), n_in = (size_t)std::max(in[0].n_items, 0);
    const nsh_arb::span s = nsh_arb::span_of(_step, _fshift, _phase, (int64_t)n_in, std::max(out[0].n_items, 0));
    const gr_complex* x = static_cast<const gr_complex*>(in[0].buffer->read_ptr());
    gr_complex* y = static_cast<gr_complex*>(out[0].buffer->write_ptr());
    _ext.resize(H + n_in);
    std::memcpy(_ext.data() + H, x, n_in * sizeof(gr_complex));
    for (int64_t n = 0; n < s.n_out; ++n) {
        const unsigned __int128 pos = (unsigned __int128)_phase + (unsigned __int128)(uint64_t)n * _step;
        const uint64_t k = (uint64_t)(pos >> 32);
        const float mu = (float)((uint32_t)pos >> 8) * 0x1p-24f;
        const gr_complex* w = _ext.data() + H + (size_t)(k >> _fshift); // x[i(n)]
        float re = 0.f, im = 0.f;
        for (int t = (int)(k & (uint64_t)(F - 1)), q = 0; t < L; t += F, ++q) { // none beyond L
            const float c = std::fmaf(mu, _diff[t], _taps[t]);
            re = std::fmaf(c, w[-q].real(), re);
            im = std::fmaf(c, w[-q].imag(), im);
        }
        y[n] = gr_complex(re, im);
    }
    std::memmove(_ext.data(), _ext.data() + s.n_consumed, H * sizeof(gr_complex)); // the Q-1 raw inputs before in[c]
    _ext.resize(H);
    _phase = s.phase_next;
    if (s.n_out == 0 && s.n_consumed > 0) ++_advances;
    out[0].n_produced = (int)s.n_out;
    in[0].n_consumed = (int)s.n_consumed;
    return work_return_code_t::WORK_OK;
}

// ---- fft_filter_ccc: the direct form in double ---------------------------------------------------
fft_filter_ccc::fft_filter_ccc(const std::vector<gr_complex>& taps) : sync_block("fft_filter_ccc"), _taps(taps)
{
    if (taps.empty() || taps.size() > 4096) throw std::invalid_argument("fft_filter_ccc: 1 to 4096 taps");
    for (auto& t : taps)
        if (!std::isfinite(t.real()) || !std::isfinite(t.imag())) throw std::invalid_argument("fft_filter_ccc: a tap is not finite");
}

bool fft_filter_ccc::start()
{
    _ext.assign(_taps.size() - 1, gr_complex(0, 0)); // zero history at stream start
    return block::start();
}

work_return_code_t fft_filter_ccc::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const size_t n = (size_t)out[0].n_items, L = _taps.size();
    gr_complex* y = static_cast<gr_complex*>(out[0].buffer->write_ptr());
    if (_ext.size() < L - 1) _ext.assign(L - 1, gr_complex(0, 0)); // not started: zeros
    _ext.resize(L - 1 + n);
    std::memcpy(_ext.data() + (L - 1), in[0].buffer->read_ptr(), n * sizeof(gr_complex));
    for (size_t i = 0; i < n; ++i) {
        const gr_complex* x = _ext.data() + (L - 1) + i; // x[-k] = sample i - k
        double re = 0, im = 0;
        for (size_t k = 0; k < L; ++k) {
            const double hr = _taps[k].real(), hi = _taps[k].imag(), xr = (x - k)->real(), xi = (x - k)->imag();
            re += hr * xr - hi * xi;
            im += hr * xi + hi * xr;
        }
        y[i] = gr_complex((float)re, (float)im);
    }
    std::memmove(_ext.data(), _ext.data() + n, (L - 1) * sizeof(gr_complex)); // the last L-1 inputs
    _ext.resize(L - 1);
    out[0].n_produced = (int)n;
    return work_return_code_t::WORK_OK;
}

// ---- freq_xlating_fft_filter_ccc: the direct form in double, the 64-bit phase ----------------------
freq_xlating_fft_filter_ccc::freq_xlating_fft_filter_ccc(int decim, const std::vector<gr_complex>& taps, double center_freq,
                                                         double samp_rate)
    : decim_block("freq_xlating_fft_filter_ccc", (unsigned)(decim > 0 ? decim : 1)), _taps(taps), _decim(decim)
{
    if (taps.empty() || taps.size() > 4096) throw std::invalid_argument("freq_xlating_fft_filter_ccc: 1 to 4096 taps");
    for (auto& t : taps)
        if (!std::isfinite(t.real()) || !std::isfinite(t.imag()))
            throw std::invalid_argument("freq_xlating_fft_filter_ccc: a tap is not finite");
    if (decim < 1 || decim > 64 || (decim & (decim - 1)))
        throw std::invalid_argument("freq_xlating_fft_filter_ccc: decimation must be a power of two in [1, 64]");
    if (!(samp_rate > 0)) throw std::invalid_argument("freq_xlating_fft_filter_ccc: samp_rate must be positive");
    if (!std::isfinite(center_freq / samp_rate))
        throw std::invalid_argument("freq_xlating_fft_filter_ccc: the frequency must be finite");
    _inc = phase_inc_turns(-(center_freq / samp_rate));
}

bool freq_xlating_fft_filter_ccc::start()
{
    _ext.assign(_taps.size() - 1, gr_complex(0, 0)); // zero history at stream start
    _index = _first;
    return block::start();
}

work_return_code_t freq_xlating_fft_filter_ccc::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int n_out = out[0].n_items; // decim_block::do_work: in[0].n_items == D * n_out
    const int L = (int)_taps.size();
    const size_t n_in = (size_t)n_out * _decim;
    gr_complex* y = static_cast<gr_complex*>(out[0].buffer->write_ptr());
    if (_ext.size() < (size_t)(L - 1)) _ext.assign(L - 1, gr_complex(0, 0)); // not started: zeros
    _ext.resize((size_t)(L - 1) + n_in);
    std::memcpy(_ext.data() + (L - 1), in[0].buffer->read_ptr(), n_in * sizeof(gr_complex));
    // rotate every sample of the window once (the raw history is rotated again with its own phase)
    std::vector<std::complex<double>> rot(_ext.size());
    for (size_t i = 0; i < _ext.size(); ++i) {
        double s, c;
        phase_sincos((_index + (uint64_t)i - (uint64_t)(L - 1)) * _inc, s, c);
        const double re = _ext[i].real(), im = _ext[i].imag();
        rot[i] = std::complex<double>(re * c - im * s, re * s + im * c);
    }
    for (int m = 0; m < n_out; ++m) {
        const std::complex<double>* w = rot.data() + (size_t)m * _decim + (L - 1);
        double re = 0, im = 0;
        for (int k = 0; k < L; ++k) {
            const double hr = _taps[k].real(), hi = _taps[k].imag(), xr = w[-k].real(), xi = w[-k].imag();
            re += hr * xr - hi * xi;
            im += hr * xi + hi * xr;
        }
        y[m] = gr_complex((float)re, (float)im);
    }
    std::memmove(_ext.data(), _ext.data() + n_in, (size_t)(L - 1) * sizeof(gr_complex)); // the last L-1 raw inputs
    _ext.resize((size_t)(L - 1));
    _index += (uint64_t)n_in;
    out[0].n_produced = n_out;
    return work_return_code_t::WORK_OK;
}

// ---- psd_vcf: radix-2 in double, squares and sum in double, rounded once --------------------------
psd_vcf::psd_vcf(size_t fft_size, size_t navg, const std::vector<float>& window, bool shift, float scale, bool db)
    : decim_block("psd_vcf", (unsigned)navg), _fft_size(fft_size), _navg(navg), _shift(shift), _db(db), _scale(scale), _window(window)
{
    if (fft_size < 16 || fft_size > 8192 || (fft_size & (fft_size - 1)))
        throw std::invalid_argument("psd_vcf: fft_size must be a power of two in [16, 8192]");
    if (navg < 1 || navg > 65536) throw std::invalid_argument("psd_vcf: navg must be in [1, 65536]");
    if (!window.empty() && window.size() != fft_size) throw std::invalid_argument("psd_vcf: the window must have fft_size entries");
    for (float w : window)
        if (!std::isfinite(w)) throw std::invalid_argument("psd_vcf: a window entry is not finite");
    if (!std::isfinite(scale) || scale < 0.f) throw std::invalid_argument("psd_vcf: scale must be finite and > 0 (0: 1 / navg)");
    if (scale == 0.f) _scale = 1.f / (float)navg;
    _tw.resize(fft_size / 2);
    for (size_t t = 0; t < fft_size / 2; ++t) {
        const double a = -2.0 * M_PI * (double)t / (double)fft_size;
        _tw[t] = { std::cos(a), std::sin(a) };
    }
    _a.resize(fft_size);
    _sum.resize(fft_size);
}

work_return_code_t psd_vcf::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const size_t N = _fft_size, H = N / 2;
    const gr_complex* x = static_cast<const gr_complex*>(in[0].buffer->read_ptr());
    float* y = static_cast<float*>(out[0].buffer->write_ptr());
    size_t bits = 0;
    while (((size_t)1 << bits) < N) ++bits;
    for (int j = 0; j < out[0].n_items; ++j, y += N) {
        std::fill(_sum.begin(), _sum.end(), 0.0);
        for (size_t f = 0; f < _navg; ++f, x += N) {
            for (size_t n = 0; n < N; ++n) {
                const float w = _window.empty() ? 1.f : _window[n];
                size_t rev = 0;
                for (size_t b = 0; b < bits; ++b) rev |= ((n >> b) & 1) << (bits - 1 - b);
                _a[rev] = { (double)(x[n].real() * w), (double)(x[n].imag() * w) };
            }
            for (size_t len = 2; len <= N; len <<= 1)
                for (size_t i = 0; i < N; i += len)
                    for (size_t k = 0; k < len / 2; ++k) {
                        const std::complex<double> u = _a[i + k], v = _a[i + k + len / 2] * _tw[k * (N / len)];
                        _a[i + k] = u + v;
                        _a[i + k + len / 2] = u - v;
                    }
            for (size_t k = 0; k < N; ++k) _sum[k] += std::norm(_a[k]);
        }
        for (size_t k = 0; k < N; ++k) {
            const double p = (double)_scale * _sum[_shift ? k ^ H : k];
            y[k] = (float)(_db ? 10.0 * std::log10(p) : p);
        }
    }
    out[0].n_produced = out[0].n_items;
    return work_return_code_t::WORK_OK;
}

const char* cpu_isa()
{
    switch (g_isa) {
    case isa::avx512: return "avx512f+fma";
    case isa::avx2: return "avx2+fma";
    default: return "x86-64 baseline (sse2)";
    }
}

} // namespace blocks
} // namespace gr
