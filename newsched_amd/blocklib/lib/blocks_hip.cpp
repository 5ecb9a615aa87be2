// gr::hip::* block work() implementations: argument plumbing from block_work_io to the
// libnsh_hip.so C-ABI on the thread's HIP stream. Nonzero codes throw (hip::check).
#include <gnuradio/run_trace.hpp>
#include <gnuradio/blocklib/hip/arith.hpp>
#include <gnuradio/blocklib/hip/copy.hpp>
#include <gnuradio/blocklib/hip/fft.hpp>
#include <gnuradio/blocklib/hip/fft_filter.hpp>
#include <gnuradio/blocklib/hip/fir_filter_cascade_ccf.hpp>
#include <gnuradio/blocklib/hip/fir_filter_ccf.hpp>
#include <gnuradio/blocklib/hip/freq_xlating_fft_filter_ccc.hpp>
#include <gnuradio/blocklib/hip/freq_xlating_fir_filter_ccf.hpp>
#include <gnuradio/blocklib/hip/multiply_const.hpp>
#include <gnuradio/blocklib/hip/pfb_arb_resampler_ccf.hpp>
#include <gnuradio/blocklib/hip/pfb_channelizer_ccf.hpp>
#include <gnuradio/blocklib/hip/pfb_synthesizer_ccf.hpp>
#include <gnuradio/blocklib/hip/psd.hpp>
#include <gnuradio/blocklib/hip/rational_resampler_ccf.hpp>
#include <gnuradio/blocklib/hip/rotator_cc.hpp>
#include <gnuradio/blocklib/hip/synth_source.hpp>
#include <gnuradio/hip_context.hpp>

#include <algorithm>
#include <cmath>
#include <stdexcept>

#include "../../csrc/nsh_arb_span.hpp"
#include "nsh_hip.h"

namespace gr {
namespace hip {

work_return_code_t copy::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const size_t n = (size_t)out[0].n_items;
    for (size_t l = 0; l < d_load; ++l)
        check(nsh_copy(in[0].buffer->read_ptr(), out[0].buffer->write_ptr(), n * d_batch_size * sizeof(gr_complex),
                       current_stream()),
              "hip::copy");
    out[0].n_produced = out[0].n_items;
    return work_return_code_t::WORK_OK;
}

template <>
work_return_code_t multiply_const<gr_complex>::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    check(nsh_mul_const_cc((const float*)in[0].buffer->read_ptr(), (float*)out[0].buffer->write_ptr(),
                           (int64_t)out[0].n_items * (int64_t)d_vlen, d_k.real(), d_k.imag(), current_stream()),
          "hip::multiply_const_cc");
    out[0].n_produced = out[0].n_items;
    return work_return_code_t::WORK_OK;
}

template <>
work_return_code_t multiply_const<float>::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    check(nsh_mul_const_ff((const float*)in[0].buffer->read_ptr(), (float*)out[0].buffer->write_ptr(),
                           (int64_t)out[0].n_items * (int64_t)d_vlen, d_k, current_stream()),
          "hip::multiply_const_ff");
    out[0].n_produced = out[0].n_items;
    return work_return_code_t::WORK_OK;
}
template class multiply_const<gr_complex>;
template class multiply_const<float>;

multiply_const_vcc::multiply_const_vcc(const std::vector<gr_complex>& k) : sync_block("multiply_const_vcc (hip)"), d_k(k)
{
    if (k.empty()) throw std::invalid_argument("hip::multiply_const_vcc: k must not be empty");
}
multiply_const_vcc::~multiply_const_vcc()
{
    if (d_kdev) nsh_free(d_kdev);
}
bool multiply_const_vcc::start()
{
    if (!d_kdev) { // the constant lives on the device of the thread that runs the block
        check(nsh_malloc(current_device(), d_k.size() * sizeof(gr_complex), &d_kdev), "hip::multiply_const_vcc");
        check(nsh_memcpy_async(d_kdev, d_k.data(), d_k.size() * sizeof(gr_complex), NSH_H2D, current_stream()),
              "hip::multiply_const_vcc");
        check(nsh_stream_sync(current_stream()), "hip::multiply_const_vcc");
    }
    return sync_block::start();
}
work_return_code_t multiply_const_vcc::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    check(nsh_mul_const_vcc((const float*)in[0].buffer->read_ptr(), (float*)out[0].buffer->write_ptr(),
                            (const float*)d_kdev, (int)d_k.size(), out[0].n_items, current_stream()),
          "hip::multiply_const_vcc");
    out[0].n_produced = out[0].n_items;
    return work_return_code_t::WORK_OK;
}

work_return_code_t multiply_const_chain_cc::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    std::vector<float> k;
    k.reserve(2 * d_ks.size());
    for (auto& c : d_ks) {
        k.push_back(c.real());
        k.push_back(c.imag());
    }
    check(nsh_mul_const_chain_cc((const float*)in[0].buffer->read_ptr(), (float*)out[0].buffer->write_ptr(),
                                 (int64_t)out[0].n_items * (int64_t)d_vlen, k.data(), (int)d_ks.size(), current_stream()),
          "hip::multiply_const_chain_cc");
    out[0].n_produced = out[0].n_items;
    return work_return_code_t::WORK_OK;
}

template <int OP>
work_return_code_t arith_cc<OP>::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int64_t n = (int64_t)out[0].n_items * (int64_t)_vlen;
    float* o = (float*)out[0].buffer->write_ptr();
    void* s = current_stream();
    if (_nports == 1) {
        check(nsh_copy(in[0].buffer->read_ptr(), o, (size_t)n * 8, s), "hip::arith_cc");
    } else {
        for (size_t p = 1; p < _nports; ++p) {
            const float* a = p == 1 ? (const float*)in[0].buffer->read_ptr() : o;
            const float* b = (const float*)in[p].buffer->read_ptr();
            check(OP == 0 ? nsh_add_cc(a, b, o, n, s) : nsh_mul_cc(a, b, o, n, s), OP == 0 ? "hip::add_cc" : "hip::multiply_cc");
        }
    }
    out[0].n_produced = out[0].n_items;
    return work_return_code_t::WORK_OK;
}
template class arith_cc<0>;
template class arith_cc<1>;

// ---- history and timing state of the FIR-family blocks (fir_stream_state.hpp) -------------
void history_state::release()
{
    if (_plan) _destroy(_plan);
    for (auto& h : _hist)
        if (h) nsh_free(h);
    _plan = nullptr;
    _hist[0] = _hist[1] = nullptr;
}

void history_state::prepare(int dev, const plan_factory& make_plan)
{
    if (on_other_device(dev)) release();
    if (_plan) return;
    _dev = dev;
    _len = make_plan(dev, &_plan);
    const size_t hbytes = std::max<size_t>(_len, 1) * sizeof(gr_complex);
    check(nsh_malloc(dev, hbytes, &_hist[0]), (_who + " history").c_str());
    check(nsh_malloc(dev, hbytes, &_hist[1]), (_who + " history").c_str());
}

void history_state::begin_run(void* stream)
{
    _zero = true;
    if (!_init.empty()) {
        if (_init.size() != _len) throw std::invalid_argument(_who + ": initial history must have ntaps-1 samples");
        const std::string what = _who + " history load";
        check(nsh_memcpy_async(_hist[0], _init.data(), _len * sizeof(gr_complex), NSH_H2D, stream), what.c_str());
        check(nsh_stream_sync(stream), what.c_str()); // host vector must outlive the copy
        _zero = false;
    }
    _cur = 0;
}

static bool timing_by_records()
{
    static const bool r = [] {
        const char* v = std::getenv("NSH_FIR_TIMING");
        return v && std::string(v) == "records";
    }();
    return r;
}

void event_pool::release()
{
    for (auto& e : _ev) {
        nsh_event_destroy(e.first);
        nsh_event_destroy(e.second);
    }
    _ev.clear();
    _used = 0;
}

void event_pool::arm(void* stream)
{
    if (_used == _ev.size()) {
        std::pair<void*, void*> p{ nullptr, nullptr };
        check(nsh_event_create(&p.first), _what.c_str());
        check(nsh_event_create(&p.second), _what.c_str());
        _ev.push_back(p);
    }
    const auto& ev = _ev[_used++];
    if (timing_by_records())
        check(nsh_event_record(ev.first, stream), _what.c_str());
    else // the launch records both events itself (nsh_time_next_launch)
        check(nsh_time_next_launch(ev.first, ev.second), _what.c_str());
}

void event_pool::recorded(void* stream)
{
    if (timing_by_records()) check(nsh_event_record(_ev[_used - 1].second, stream), _what.c_str());
}

double event_pool::sum_ms(double total)
{
    for (size_t i = 0; i < _used; ++i) {
        float ms = 0;
        check(nsh_event_sync(_ev[i].second), _what.c_str());
        check(nsh_event_elapsed_ms(_ev[i].first, _ev[i].second, &ms), _what.c_str());
        total += ms;
    }
    return total;
}

// ---- FIR ---------------------------------------------------------------------------
fir_filter_ccf::fir_filter_ccf(const std::vector<float>& taps, int decim, int algo)
    : decim_block("fir_filter_ccf (hip)", (unsigned)decim),
      _ev("hip::fir_filter_ccf"),
      _taps(taps),
      _decim(decim),
      _algo(algo),
      _state("hip::fir_filter_ccf", nsh_fir_plan_destroy)
{
    if (taps.empty()) throw std::invalid_argument("hip::fir_filter_ccf: no taps");
    if (decim != 1 && decim != 2 && decim != 4 && decim != 8 && decim != 16)
        throw std::invalid_argument("hip::fir_filter_ccf: decimation must be 1, 2, 4, 8 or 16");
}

fir_filter_ccf::~fir_filter_ccf() = default;

int fir_filter_ccf::algo() const { return _state.plan() ? nsh_fir_plan_algo(_state.plan()) : _algo; }
std::string fir_filter_ccf::kernel() const { return _state.plan() ? nsh_fir_plan_kernel(_state.plan()) : std::string(); }

bool fir_filter_ccf::start()
{
    const int dev = current_device();
    if (_state.on_other_device(dev)) _ev.release(); // the events belong to the old device too
    _state.prepare(dev, [this](int d, void** plan) {
        check(nsh_fir_plan_create(d, _taps.data(), (int)_taps.size(), _decim, _algo, plan), "hip::fir_filter_ccf plan");
        return _taps.size() - 1;
    });
    _state.begin_run(current_stream());
    // the events of earlier runs are folded into the total when it is read (kernel_ms), not here:
    // nothing per run but the two records per launch; a long unread series is folded at 4096
    if (_ev.pending() >= 4096) kernel_ms();
    return block::start();
}

work_return_code_t fir_filter_ccf::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int n_out = out[0].n_items; // decim_block::do_work: in[0].n_items == D * n_out
    void* s = current_stream();
    const bool timed = _timing && _launches % (uint64_t)_stride == 0;
    if (timed) _ev.arm(s);
    NSR_RT(4);
    check(nsh_fir_ccf(_state.plan(), (const float*)in[0].buffer->read_ptr(), _state.hist_in(), _state.hist_out(),
                      (float*)out[0].buffer->write_ptr(), n_out, s),
          "hip::fir_filter_ccf");
    if (timed) {
        _ev.recorded(s);
        _timed_samples += (uint64_t)n_out;
        ++_timed_launches;
    }
    NSR_RT(5);
    _state.flip();
    ++_launches;
    out[0].n_produced = n_out;
    return work_return_code_t::WORK_OK;
}

double fir_filter_ccf::kernel_ms()
{
    _done_ms = _ev.sum_ms(_done_ms);
    _ev.reuse(); // folded: the events are reused by the next launches
    return _done_ms;
}

// ---- fused decimating FIR chain -----------------------------------------------------
namespace {
int total_decim(const std::vector<fir_filter_cascade_ccf::stage>& st)
{
    int64_t d = 1;
    for (auto& s : st) d *= s.second > 0 ? s.second : 0;
    return d > 64 ? 64 : (int)d;
}
} // namespace

bool fir_filter_cascade_ccf::supported(const std::vector<stage>& st)
{
    if (st.empty()) return false;
    const int D = total_decim(st);
    if (D != 8 && D != 16) return false;
    int64_t len = 1, dacc = 1; // composite length 1 + sum (L_s - 1) prod_{t<s} D_t
    for (auto& s : st) {
        if (s.first.empty()) return false;
        for (float v : s.first)
            if (!std::isfinite(v)) return false;
        len += (int64_t)(s.first.size() - 1) * dacc;
        dacc *= s.second;
    }
    return (len - 1 + D - 1) / D <= 256; // nsh_fir_cascade_plan_create's limit
}

fir_filter_cascade_ccf::fir_filter_cascade_ccf(const std::vector<stage>& stages)
    : decim_block("fir_filter_cascade_ccf (hip)", (unsigned)total_decim(stages)),
      _stages(stages),
      _state("hip::fir_filter_cascade_ccf", nsh_fir_cascade_plan_destroy),
      _ev("hip::fir_filter_cascade_ccf")
{
    if (!supported(stages))
        throw std::invalid_argument("hip::fir_filter_cascade_ccf: needs total decimation 8 or 16, finite taps and "
                                    "ceil((len(heq)-1)/D) <= 256");
}

fir_filter_cascade_ccf::~fir_filter_cascade_ccf() = default;

std::string fir_filter_cascade_ccf::kernel() const
{
    return _state.plan() ? nsh_fir_cascade_kernel(_state.plan()) : std::string();
}

bool fir_filter_cascade_ccf::start()
{
    const int dev = current_device();
    if (_state.on_other_device(dev)) _ev.release(); // the events belong to the old device too
    _state.prepare(dev, [this](int d, void** plan) {
        std::vector<const float*> tp;
        std::vector<int> nt, dc;
        for (auto& s : _stages) {
            tp.push_back(s.first.data());
            nt.push_back((int)s.first.size());
            dc.push_back(s.second);
        }
        check(nsh_fir_cascade_plan_create(d, tp.data(), nt.data(), dc.data(), (int)_stages.size(), plan),
              "hip::fir_filter_cascade_ccf plan");
        return (size_t)nsh_fir_cascade_hist_len(*plan);
    });
    _state.begin_run(current_stream()); // a fresh stream: the first call reads a null (zero) history
    _ev.reuse();
    _timed_samples = 0;
    return block::start();
}

work_return_code_t fir_filter_cascade_ccf::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int n_out = out[0].n_items; // decim_block::do_work: in[0].n_items == D * n_out
    void* s = current_stream();
    if (_timing) _ev.arm(s);
    check(nsh_fir_cascade_ccf(_state.plan(), (const float*)in[0].buffer->read_ptr(), _state.hist_in(), _state.hist_out(),
                              (float*)out[0].buffer->write_ptr(), n_out, s),
          "hip::fir_filter_cascade_ccf");
    if (_timing) {
        _ev.recorded(s);
        _timed_samples += (uint64_t)n_out;
    }
    _state.flip();
    ++_launches;
    out[0].n_produced = n_out;
    return work_return_code_t::WORK_OK;
}

double fir_filter_cascade_ccf::kernel_ms() { return _ev.sum_ms(); }

// ---- rotator / frequency-translating FIR ----------------------------------------------
work_return_code_t rotator_cc::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int n = out[0].n_items;
    check(nsh_rotate_cc((const float*)in[0].buffer->read_ptr(), (float*)out[0].buffer->write_ptr(), n, _inc, _index,
                        current_stream()),
          "hip::rotator_cc");
    _index += (uint64_t)n;
    ++_launches;
    out[0].n_produced = n;
    return work_return_code_t::WORK_OK;
}

freq_xlating_fir_filter_ccf::freq_xlating_fir_filter_ccf(int decim, const std::vector<float>& taps, double center_freq,
                                                         double samp_rate)
    : decim_block("freq_xlating_fir_filter_ccf (hip)", (unsigned)(decim > 0 ? decim : 1)),
      _taps(taps),
      _decim(decim),
      _state("hip::freq_xlating_fir_filter_ccf", nsh_fir_xlat_plan_destroy)
{
    if (taps.empty() || taps.size() > 1024) throw std::invalid_argument("hip::freq_xlating_fir_filter_ccf: 1 to 1024 taps");
    if (decim < 1 || decim > 64) throw std::invalid_argument("hip::freq_xlating_fir_filter_ccf: decimation must be in [1, 64]");
    if (!(samp_rate > 0)) throw std::invalid_argument("hip::freq_xlating_fir_filter_ccf: samp_rate must be positive");
    _freq_norm = center_freq / samp_rate;
    if (!std::isfinite(_freq_norm)) throw std::invalid_argument("hip::freq_xlating_fir_filter_ccf: the frequency must be finite");
}

freq_xlating_fir_filter_ccf::~freq_xlating_fir_filter_ccf() = default;

uint64_t freq_xlating_fir_filter_ccf::phase_inc() const
{
    uint64_t inc = 0;
    if (_state.plan()) nsh_fir_xlat_phase_inc(_state.plan(), &inc);
    return inc;
}
std::string freq_xlating_fir_filter_ccf::kernel() const
{
    return _state.plan() ? nsh_fir_xlat_kernel(_state.plan()) : std::string();
}

bool freq_xlating_fir_filter_ccf::start()
{
    _state.prepare(current_device(), [this](int d, void** plan) {
        check(nsh_fir_xlat_plan_create(d, _taps.data(), (int)_taps.size(), _decim, _freq_norm, plan),
              "hip::freq_xlating_fir_filter_ccf plan");
        return _taps.size() - 1;
    });
    _state.begin_run(current_stream());
    _index = _first;
    return block::start();
}

work_return_code_t freq_xlating_fir_filter_ccf::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int n_out = out[0].n_items; // decim_block::do_work: in[0].n_items == D * n_out
    check(nsh_fir_xlat_ccf(_state.plan(), (const float*)in[0].buffer->read_ptr(), _state.hist_in(), _state.hist_out(),
                           (float*)out[0].buffer->write_ptr(), n_out, _index, current_stream()),
          "hip::freq_xlating_fir_filter_ccf");
    _state.flip();
    _index += (uint64_t)n_out * (uint64_t)_decim;
    ++_launches;
    out[0].n_produced = n_out;
    return work_return_code_t::WORK_OK;
}

// ---- polyphase filterbank channelizer -------------------------------------------------
pfb_channelizer_ccf::pfb_channelizer_ccf(int nchans, const std::vector<float>& taps)
    : decim_block("pfb_channelizer_ccf (hip)", (unsigned)(nchans > 0 ? nchans : 1)),
      _taps(taps),
      _nchans(nchans),
      _state("hip::pfb_channelizer_ccf", nsh_pfb_plan_destroy)
{
    if (taps.empty() || taps.size() > 1024) throw std::invalid_argument("hip::pfb_channelizer_ccf: 1 to 1024 taps");
    if (nchans < 2 || nchans > 64 || (nchans & (nchans - 1)))
        throw std::invalid_argument("hip::pfb_channelizer_ccf: nchans must be a power of two in [2, 64]");
    if ((taps.size() + (size_t)nchans - 1) / (size_t)nchans > 32)
        throw std::invalid_argument("hip::pfb_channelizer_ccf: at most 32 taps per branch");
}

pfb_channelizer_ccf::~pfb_channelizer_ccf() = default;

std::string pfb_channelizer_ccf::kernel() const { return _state.plan() ? nsh_pfb_kernel(_state.plan()) : std::string(); }

bool pfb_channelizer_ccf::start()
{
    _state.prepare(current_device(), [this](int d, void** plan) {
        check(nsh_pfb_plan_create(d, _taps.data(), (int)_taps.size(), _nchans, plan), "hip::pfb_channelizer_ccf plan");
        return _taps.size() - 1;
    });
    _state.begin_run(current_stream());
    return block::start();
}

work_return_code_t pfb_channelizer_ccf::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int n_out = out[0].n_items; // decim_block::do_work: in[0].n_items == M * n_out
    check(nsh_pfb_channelizer_ccf(_state.plan(), (const float*)in[0].buffer->read_ptr(), _state.hist_in(), _state.hist_out(),
                                  (float*)out[0].buffer->write_ptr(), n_out, current_stream()),
          "hip::pfb_channelizer_ccf");
    _state.flip();
    ++_launches;
    out[0].n_produced = n_out;
    return work_return_code_t::WORK_OK;
}

// ---- polyphase synthesis filterbank ----------------------------------------------------
pfb_synthesizer_ccf::pfb_synthesizer_ccf(int nchans, const std::vector<float>& taps)
    : resamp_block("pfb_synthesizer_ccf (hip)", (unsigned)(nchans > 0 ? nchans : 1), 1),
      _taps(taps),
      _nchans(nchans),
      _state("hip::pfb_synthesizer_ccf", nsh_pfb_synth_plan_destroy)
{
    if (taps.empty() || taps.size() > 1024) throw std::invalid_argument("hip::pfb_synthesizer_ccf: 1 to 1024 taps");
    if (nchans < 2 || nchans > 64 || (nchans & (nchans - 1)))
        throw std::invalid_argument("hip::pfb_synthesizer_ccf: nchans must be a power of two in [2, 64]");
    if ((taps.size() + (size_t)nchans - 1) / (size_t)nchans > 32)
        throw std::invalid_argument("hip::pfb_synthesizer_ccf: at most 32 taps per branch");
}

pfb_synthesizer_ccf::~pfb_synthesizer_ccf() = default;

std::string pfb_synthesizer_ccf::kernel() const
{
    return _state.plan() ? nsh_pfb_synth_kernel(_state.plan()) : std::string();
}

bool pfb_synthesizer_ccf::start()
{
    _state.prepare(current_device(), [this](int d, void** plan) {
        check(nsh_pfb_synth_plan_create(d, _taps.data(), (int)_taps.size(), _nchans, plan), "hip::pfb_synthesizer_ccf plan");
        return ((_taps.size() + (size_t)_nchans - 1) / (size_t)_nchans - 1) * (size_t)_nchans; // Q-1 items
    });
    _state.begin_run(current_stream());
    return block::start();
}

work_return_code_t pfb_synthesizer_ccf::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int n_in = out[0].n_items / _nchans; // resamp_block::do_work: n items in, n M samples out
    check(nsh_pfb_synthesizer_ccf(_state.plan(), (const float*)in[0].buffer->read_ptr(), _state.hist_in(), _state.hist_out(),
                                  (float*)out[0].buffer->write_ptr(), n_in, current_stream()),
          "hip::pfb_synthesizer_ccf");
    _state.flip();
    ++_launches;
    out[0].n_produced = n_in * _nchans;
    return work_return_code_t::WORK_OK;
}

// ---- rational resampler ----------------------------------------------------------------
rational_resampler_ccf::rational_resampler_ccf(int interp, int decim, const std::vector<float>& taps)
    : resamp_block("rational_resampler_ccf (hip)", (unsigned)(interp > 0 ? interp : 1), (unsigned)(decim > 0 ? decim : 1)),
      _taps(taps),
      _interp(interp),
      _decim(decim),
      _state("hip::rational_resampler_ccf", nsh_resamp_plan_destroy)
{
    if (taps.empty() || taps.size() > 1024) throw std::invalid_argument("hip::rational_resampler_ccf: ntaps must be in [1, 1024]");
    if (interp < 1 || interp > 64) throw std::invalid_argument("hip::rational_resampler_ccf: interpolation must be in [1, 64]");
    if (decim < 1 || decim > 64) throw std::invalid_argument("hip::rational_resampler_ccf: decimation must be in [1, 64]");
}

rational_resampler_ccf::~rational_resampler_ccf() = default;

std::string rational_resampler_ccf::kernel() const
{
    return _state.plan() ? nsh_resamp_kernel(_state.plan()) : std::string();
}

bool rational_resampler_ccf::start()
{
    _state.prepare(current_device(), [this](int d, void** plan) {
        check(nsh_resamp_plan_create(d, _taps.data(), (int)_taps.size(), _interp, _decim, plan),
              "hip::rational_resampler_ccf plan");
        return (size_t)nsh_resamp_history(*plan);
    });
    _state.begin_run(current_stream());
    return block::start();
}

work_return_code_t rational_resampler_ccf::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int n_units = out[0].n_items / _interp; // resamp_block::do_work: n D inputs, n I outputs
    check(nsh_resamp_ccf(_state.plan(), (const float*)in[0].buffer->read_ptr(), _state.hist_in(), _state.hist_out(),
                         (float*)out[0].buffer->write_ptr(), n_units, current_stream()),
          "hip::rational_resampler_ccf");
    _state.flip();
    ++_launches;
    out[0].n_produced = n_units * _interp;
    return work_return_code_t::WORK_OK;
}

// ---- arbitrary-rate polyphase resampler ------------------------------------------------
pfb_arb_resampler_ccf::pfb_arb_resampler_ccf(double rate, const std::vector<float>& taps, unsigned filter_size)
    : block("pfb_arb_resampler_ccf (hip)"),
      _rate(rate),
      _taps(taps),
      _nfilt(filter_size),
      _state("hip::pfb_arb_resampler_ccf", nsh_arb_plan_destroy)
{
    _fshift = filter_size <= 64 ? nsh_arb::filt_shift((int)filter_size) : -1;
    if (_fshift < 0) throw std::invalid_argument("hip::pfb_arb_resampler_ccf: nfilt must be a power of two in [2, 64]");
    if (taps.empty() || taps.size() > 2048) throw std::invalid_argument("hip::pfb_arb_resampler_ccf: ntaps must be in [1, 2048]");
    if (!nsh_arb::rate_ok(rate)) throw std::invalid_argument("hip::pfb_arb_resampler_ccf: rate must be finite and in [1/64, 64]");
    _step = nsh_arb::step_of(rate, (int)filter_size);
}

pfb_arb_resampler_ccf::~pfb_arb_resampler_ccf() = default;

std::string pfb_arb_resampler_ccf::kernel() const { return _state.plan() ? nsh_arb_kernel(_state.plan()) : std::string(); }

bool pfb_arb_resampler_ccf::start()
{
    _state.prepare(current_device(), [this](int d, void** plan) {
        check(nsh_arb_plan_create(d, _taps.data(), (int)_taps.size(), (int)_nfilt, _rate, plan), "hip::pfb_arb_resampler_ccf plan");
        return (size_t)nsh_arb_history(*plan);
    });
    _state.begin_run(current_stream());
    _phase = _phase0;
    return block::start();
}

work_return_code_t pfb_arb_resampler_ccf::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int64_t n_in = std::max(in[0].n_items, 0);
    const nsh_arb::span s = nsh_arb::span_of(_step, _fshift, _phase, n_in, std::max(out[0].n_items, 0));
    // n_out = 0 advances: the kernel only hands the history on
    check(nsh_arb_resamp_ccf(_state.plan(), (const float*)in[0].buffer->read_ptr(), n_in, _state.hist_in(), _state.hist_out(),
                             (float*)out[0].buffer->write_ptr(), s.n_out, _phase, current_stream()),
          "hip::pfb_arb_resampler_ccf");
    if (n_in > 0 && (s.n_out > 0 || nsh_arb_history(_state.plan()) > 0)) { // a launch: it wrote hist_out
        _state.flip();
        ++_launches;
    }
    _phase = s.phase_next;
    if (s.n_out == 0 && s.n_consumed > 0) ++_advances;
    out[0].n_produced = (int)s.n_out;
    in[0].n_consumed = (int)s.n_consumed;
    return work_return_code_t::WORK_OK;
}

// ---- FFT ---------------------------------------------------------------------------
fft_vcc::fft_vcc(size_t fft_size, bool forward, const std::vector<float>& window, bool shift)
    : sync_block(forward ? "fft_vcc (hip)" : "ifft_vcc (hip)"), _fft_size(fft_size), _forward(forward), _shift(shift), _window(window)
{
    if (fft_size < 16 || fft_size > 8192 || (fft_size & (fft_size - 1)))
        throw std::invalid_argument("hip::fft_vcc: fft_size must be a power of two in [16, 8192]");
    if (!window.empty() && window.size() != fft_size)
        throw std::invalid_argument("hip::fft_vcc: the window must have fft_size entries");
}
fft_vcc::~fft_vcc() { nsh_fft_plan_destroy(_plan); }
bool fft_vcc::start()
{
    const int dev = current_device();
    if (_plan && _plan_dev != dev) {
        nsh_fft_plan_destroy(_plan);
        _plan = nullptr;
    }
    if (!_plan) {
        check(nsh_fft_plan_create(dev, (int)_fft_size, _forward ? 0 : 1, _window.empty() ? nullptr : _window.data(), _shift ? 1 : 0,
                                  &_plan),
              "hip::fft_vcc plan");
        _plan_dev = dev;
    }
    return sync_block::start();
}

work_return_code_t fft_vcc::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    check(nsh_fft_c2c(_plan, (const float*)in[0].buffer->read_ptr(), (float*)out[0].buffer->write_ptr(), out[0].n_items,
                      current_stream()),
          "hip::fft_vcc");
    out[0].n_produced = out[0].n_items;
    return work_return_code_t::WORK_OK;
}

channelizer_vcc::channelizer_vcc(const std::vector<gr_complex>& w) : sync_block("channelizer_vcc (hip)"), _w(w)
{
    if (w.size() != 1024) throw std::invalid_argument("hip::channelizer_vcc: w must have 1024 bins");
}
channelizer_vcc::~channelizer_vcc()
{
    if (_wdev) nsh_free(_wdev);
}
bool channelizer_vcc::start()
{
    if (!_wdev) {
        check(nsh_malloc(current_device(), _w.size() * sizeof(gr_complex), &_wdev), "hip::channelizer_vcc");
        check(nsh_memcpy_async(_wdev, _w.data(), _w.size() * sizeof(gr_complex), NSH_H2D, current_stream()),
              "hip::channelizer_vcc");
        check(nsh_stream_sync(current_stream()), "hip::channelizer_vcc");
    }
    return sync_block::start();
}
work_return_code_t channelizer_vcc::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    check(nsh_channelizer1024((const float*)in[0].buffer->read_ptr(), (float*)out[0].buffer->write_ptr(),
                              (const float*)_wdev, out[0].n_items, current_stream()),
          "hip::channelizer_vcc");
    out[0].n_produced = out[0].n_items;
    return work_return_code_t::WORK_OK;
}

// ---- overlap-save FIR with complex taps ---------------------------------------------------
// What the overlap-save plans (nsh_fft_filter_plan_create, nsh_fft_xlat_plan_create) refuse, in
// their order; between: what a plan checks after the taps and before the frame size.
template <class F>
static void check_ols_args(const std::string& name, const std::vector<gr_complex>& taps, size_t fft_size, F between)
{
    if (taps.empty() || taps.size() > 4096) throw std::invalid_argument(name + ": 1 to 4096 taps");
    for (auto& t : taps)
        if (!std::isfinite(t.real()) || !std::isfinite(t.imag())) throw std::invalid_argument(name + ": a tap is not finite");
    between();
    if (fft_size != 0 && fft_size != 1024 && fft_size != 2048 && fft_size != 4096 && fft_size != 8192)
        throw std::invalid_argument(name + ": fft_size must be 0, 1024, 2048, 4096 or 8192");
    if (fft_size && taps.size() > fft_size / 2) throw std::invalid_argument(name + ": at most fft_size / 2 taps");
}

fft_filter_ccc::fft_filter_ccc(const std::vector<gr_complex>& taps, size_t fft_size, const char* name)
    : sync_block(name), _taps(taps), _fft_size(fft_size), _state("hip::fft_filter_ccc", nsh_fft_filter_plan_destroy),
      _ev("hip::fft_filter_ccc")
{
    check_ols_args("hip::fft_filter_ccc", taps, fft_size, [] {});
}

fft_filter_ccc::~fft_filter_ccc() = default;

size_t fft_filter_ccc::fft_size() const { return _state.plan() ? (size_t)nsh_fft_filter_fft_size(_state.plan()) : _fft_size; }
std::string fft_filter_ccc::kernel() const { return _state.plan() ? nsh_fft_filter_kernel(_state.plan()) : std::string(); }

bool fft_filter_ccc::start()
{
    const int dev = current_device();
    if (_state.on_other_device(dev)) _ev.release(); // the events belong to the old device too
    _state.prepare(dev, [this](int d, void** plan) {
        check(nsh_fft_filter_plan_create(d, reinterpret_cast<const float*>(_taps.data()), (int)_taps.size(), (int)_fft_size, plan),
              "hip::fft_filter_ccc plan");
        return _taps.size() - 1;
    });
    _state.begin_run(current_stream()); // a fresh stream: the first call reads a null (zero) history
    _ev.reuse();
    _timed_samples = 0;
    return sync_block::start();
}

work_return_code_t fft_filter_ccc::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int n = out[0].n_items;
    void* s = current_stream();
    if (_timing) _ev.arm(s);
    check(nsh_fft_filter_ccc(_state.plan(), (const float*)in[0].buffer->read_ptr(), _state.hist_in(), _state.hist_out(),
                             (float*)out[0].buffer->write_ptr(), n, s),
          "hip::fft_filter_ccc");
    if (_timing) {
        _ev.recorded(s);
        _timed_samples += (uint64_t)n;
    }
    _state.flip();
    ++_launches;
    out[0].n_produced = n;
    return work_return_code_t::WORK_OK;
}

double fft_filter_ccc::kernel_ms() { return _ev.sum_ms(); }

// ---- tune, overlap-save FIR with complex taps, decimate ---------------------------------------------
freq_xlating_fft_filter_ccc::freq_xlating_fft_filter_ccc(int decim, const std::vector<gr_complex>& taps, double center_freq,
                                                         double samp_rate, size_t fft_size, const char* name)
    : decim_block(name, (unsigned)(decim > 0 ? decim : 1)), _taps(taps), _decim(decim), _fft_size(fft_size),
      _state("hip::freq_xlating_fft_filter_ccc", nsh_fft_xlat_plan_destroy)
{
    check_ols_args("hip::freq_xlating_fft_filter_ccc", taps, fft_size, [&] {
        if (decim < 1 || decim > 64 || (decim & (decim - 1)))
            throw std::invalid_argument("hip::freq_xlating_fft_filter_ccc: decimation must be a power of two in [1, 64]");
        if (!(samp_rate > 0)) throw std::invalid_argument("hip::freq_xlating_fft_filter_ccc: samp_rate must be positive");
        _freq_norm = center_freq / samp_rate;
        if (!std::isfinite(_freq_norm))
            throw std::invalid_argument("hip::freq_xlating_fft_filter_ccc: the frequency must be finite");
    });
}

freq_xlating_fft_filter_ccc::~freq_xlating_fft_filter_ccc() = default;

size_t freq_xlating_fft_filter_ccc::fft_size() const
{
    return _state.plan() ? (size_t)nsh_fft_xlat_fft_size(_state.plan()) : _fft_size;
}
uint64_t freq_xlating_fft_filter_ccc::phase_inc() const
{
    uint64_t inc = 0;
    if (_state.plan()) nsh_fft_xlat_phase_inc(_state.plan(), &inc);
    return inc;
}
std::string freq_xlating_fft_filter_ccc::kernel() const
{
    return _state.plan() ? nsh_fft_xlat_kernel(_state.plan()) : std::string();
}

bool freq_xlating_fft_filter_ccc::start()
{
    _state.prepare(current_device(), [this](int d, void** plan) {
        check(nsh_fft_xlat_plan_create(d, reinterpret_cast<const float*>(_taps.data()), (int)_taps.size(), _decim, _freq_norm,
                                       (int)_fft_size, plan),
              "hip::freq_xlating_fft_filter_ccc plan");
        return _taps.size() - 1;
    });
    _state.begin_run(current_stream());
    _index = _first;
    return block::start();
}

work_return_code_t freq_xlating_fft_filter_ccc::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int n_out = out[0].n_items; // decim_block::do_work: in[0].n_items == D * n_out
    check(nsh_fft_xlat_ccc(_state.plan(), (const float*)in[0].buffer->read_ptr(), _state.hist_in(), _state.hist_out(),
                           (float*)out[0].buffer->write_ptr(), n_out, _index, current_stream()),
          "hip::freq_xlating_fft_filter_ccc");
    _state.flip();
    _index += (uint64_t)n_out * (uint64_t)_decim;
    ++_launches;
    out[0].n_produced = n_out;
    return work_return_code_t::WORK_OK;
}

// ---- spectrum estimate: windowed FFT, |X|^2, sum over navg frames ---------------------------------
psd_vcf::psd_vcf(size_t fft_size, size_t navg, const std::vector<float>& window, bool shift, float scale, bool db)
    : decim_block("psd_vcf (hip)", (unsigned)navg), _fft_size(fft_size), _navg(navg), _shift(shift), _db(db), _scale(scale),
      _window(window), _ev("hip::psd_vcf")
{
    // what nsh_psd_plan_create refuses, in its order
    if (fft_size < 16 || fft_size > 8192 || (fft_size & (fft_size - 1)))
        throw std::invalid_argument("hip::psd_vcf: fft_size must be a power of two in [16, 8192]");
    if (navg < 1 || navg > 65536) throw std::invalid_argument("hip::psd_vcf: navg must be in [1, 65536]");
    if (!window.empty() && window.size() != fft_size)
        throw std::invalid_argument("hip::psd_vcf: the window must have fft_size entries");
    for (float w : window)
        if (!std::isfinite(w)) throw std::invalid_argument("hip::psd_vcf: a window entry is not finite");
    if (!std::isfinite(scale) || scale < 0.f) throw std::invalid_argument("hip::psd_vcf: scale must be finite and > 0 (0: 1 / navg)");
    if (scale == 0.f) _scale = 1.f / (float)navg;
}
psd_vcf::~psd_vcf() { nsh_psd_plan_destroy(_plan); }

std::string psd_vcf::kernel() const { return _plan ? nsh_psd_kernel(_plan) : std::string(); }

bool psd_vcf::start()
{
    const int dev = current_device();
    if (_plan && _plan_dev != dev) {
        _ev.release(); // the events belong to the old device too
        nsh_psd_plan_destroy(_plan);
        _plan = nullptr;
    }
    if (!_plan) {
        check(nsh_psd_plan_create(dev, (int)_fft_size, (int)_navg, _window.empty() ? nullptr : _window.data(), _shift ? 1 : 0, _scale,
                                  _db ? 1 : 0, &_plan),
              "hip::psd_vcf plan");
        _plan_dev = dev;
    }
    _ev.reuse();
    _timed_vectors = 0;
    return block::start();
}

work_return_code_t psd_vcf::work(std::vector<block_work_input>& in, std::vector<block_work_output>& out)
{
    const int n = out[0].n_items; // decim_block::do_work: in[0].n_items == navg * n
    void* s = current_stream();
    if (_timing) _ev.arm(s);
    check(nsh_psd_cf(_plan, (const float*)in[0].buffer->read_ptr(), (float*)out[0].buffer->write_ptr(), n, s), "hip::psd_vcf");
    if (_timing) {
        _ev.recorded(s);
        _timed_vectors += (uint64_t)n;
    }
    ++_launches;
    out[0].n_produced = n;
    return work_return_code_t::WORK_OK;
}

double psd_vcf::kernel_ms() { return _ev.sum_ms(); }

// ---- synthetic source ----------------------------------------------------------------
work_return_code_t synth_source::work(std::vector<block_work_input>&, std::vector<block_work_output>& out)
{
    int64_t n = (int64_t)out[0].n_items * (int64_t)_vlen; // samples
    if (_limit) {
        const uint64_t left = _first + _limit - _index;
        if (left == 0) {
            out[0].n_produced = 0;
            return work_return_code_t::WORK_DONE;
        }
        n = std::min<int64_t>(n, (int64_t)left);
    }
    check(nsh_synth_cf32((float*)out[0].buffer->write_ptr(), n, _index, _seed, current_stream()), "hip::synth_source");
    _index += (uint64_t)n;
    out[0].n_produced = (int)(n / (int64_t)_vlen);
    if (_limit && _index >= _first + _limit) return work_return_code_t::WORK_DONE;
    return work_return_code_t::WORK_OK;
}

} // namespace hip
} // namespace gr
