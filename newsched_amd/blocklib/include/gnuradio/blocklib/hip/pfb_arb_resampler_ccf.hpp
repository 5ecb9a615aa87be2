// gr::hip::pfb_arb_resampler_ccf -- resample by an arbitrary rate r (48 kHz to 44.1 kHz, a clock that
// is off by 30 ppm, any ratio rational_resampler_ccf's I, D <= 64 cannot express): F = filter_size
// polyphase filters and their derivative filters on an exact integer phase, in one kernel launch per
// work() (nsh_arb_resamp_ccf, k_arb<R,P>: every input is read from HBM once per workgroup and every
// output written once, 8 B each). Semantics of blocks::pfb_arb_resampler_ccf; F a power of two in
// [2, 64], at most 2048 taps, 1/64 <= r <= 64.
// A plain gr::block whose output count per input is no fixed ratio: work() asks nsh_arb::span_of
// (newsched_amd/csrc/nsh_arb_span.hpp) for the outputs that fit the room and the input it was given, sets
// n_produced and n_consumed itself and carries the phase on the host; a call that can make no output
// still consumes and hands the history on. The plan and two (ceil(L / F) - 1)-sample raw-history
// buffers are created on the first start() on the partition thread; every start() resets the phase
// to set_initial_phase (default 0) and the history to zeros or set_initial_history. No
// synchronisation of its own. Measured: DESIGN.md section 4.6.
#pragma once
#include <gnuradio/block.hpp>
#include <gnuradio/blocklib/hip/fir_stream_state.hpp>

namespace gr {
namespace hip {
class pfb_arb_resampler_ccf : public block
{
public:
    using sptr = std::shared_ptr<pfb_arb_resampler_ccf>;
    static sptr make(double rate, const std::vector<float>& taps, unsigned filter_size = 32)
    {
        auto p = std::make_shared<pfb_arb_resampler_ccf>(rate, taps, filter_size);
        p->add_port(port<gr_complex>::make("in", port_direction_t::INPUT));
        p->add_port(port<gr_complex>::make("out", port_direction_t::OUTPUT));
        return p;
    }
    pfb_arb_resampler_ccf(double rate, const std::vector<float>& taps, unsigned filter_size);
    ~pfb_arb_resampler_ccf() override;
    bool start() override;
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    double relative_rate() const override { return _rate; }
    const std::vector<float>& taps() const { return _taps; }
    unsigned filter_size() const { return _nfilt; }
    uint64_t step() const { return _step; }
    uint64_t phase() const { return _phase; }
    uint64_t advancing_calls() const { return _advances; } // work() calls that consumed and made no output
    std::string kernel() const; // the kernel its work() launches (after start())
    uint64_t launches() const { return _launches; }

    // Position of the first output relative to the first input (Q32.32 filter steps) and the
    // ceil(ntaps / filter_size) - 1 RAW samples before the first input, read by start(): with both,
    // the block reproduces the tail of a longer stream bit for bit (a time shard).
    void set_initial_phase(uint64_t phase) { _phase0 = phase; }
    void set_initial_history(const std::vector<gr_complex>& h) { _state.set_initial(h); }

private:
    double _rate;
    std::vector<float> _taps;
    unsigned _nfilt;
    int _fshift = 0;
    uint64_t _step = 0, _phase0 = 0, _phase = 0;
    history_state _state;
    uint64_t _launches = 0, _advances = 0;
};
} // namespace hip
} // namespace gr
