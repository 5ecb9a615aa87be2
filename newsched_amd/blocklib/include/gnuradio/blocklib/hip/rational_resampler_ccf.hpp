// gr::hip::rational_resampler_ccf -- resample by I/D: zero-stuff by I, low-pass with L real fp32
// taps, keep every D-th sample, in one kernel launch per work() (nsh_resamp_ccf, k_resamp<R,P>: every
// input is read from HBM once and every output written once, 8 B each). Semantics of
// blocks::rational_resampler_ccf; 1 <= I, D <= 64, at most 1024 taps; larger ratios (160/147) are
// hip::pfb_arb_resampler_ccf's. D = 1 is interp_fir_filter_ccf.
// A gr::resamp_block: the plan and two (ceil(L / I) - 1)-sample raw-history buffers are created on
// the first start() on the partition thread, the history is zeroed (or loaded from
// set_initial_history) on every start().
//
// Against nsh_copy over the same 8 (n_in + n_out) bytes (kernel times on 2^27
// samples in and out together, one MI355X): (I, D, taps) = (2, 1, 63) 385 us against 169 us,
// (4, 1, 127) 444 against 170, (3, 2, 95) 366 against 168, (2, 3, 95) 466 against 168, (4, 5, 159) 424
// against 166, (64, 1, 1024) 381 against 165: 2.2 to 2.8 times the copy, 29 to 37 % of the HBM bound;
// supposed bound: one LDS read per multiply-add. Pure decimators: (1, 4, 127) 622 us, level with
// hip::freq_xlating_fir_filter_ccf at frequency 0 (643 us); (1, 64, 1024) 1115 us, twice its 558 us:
// a flowgraph that only decimates by a large D is better served by that block.
#pragma once
#include <gnuradio/blocklib/hip/fir_stream_state.hpp>
#include <gnuradio/resamp_block.hpp>

namespace gr {
namespace hip {
class rational_resampler_ccf : public resamp_block
{
public:
    using sptr = std::shared_ptr<rational_resampler_ccf>;
    static sptr make(int interp, int decim, const std::vector<float>& taps)
    {
        auto p = std::make_shared<rational_resampler_ccf>(interp, decim, taps);
        p->add_port(port<gr_complex>::make("in", port_direction_t::INPUT));
        p->add_port(port<gr_complex>::make("out", port_direction_t::OUTPUT));
        return p;
    }
    rational_resampler_ccf(int interp, int decim, const std::vector<float>& taps);
    ~rational_resampler_ccf() override;
    bool start() override;
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    int interp() const { return _interp; }
    int decim() const { return _decim; }
    const std::vector<float>& taps() const { return _taps; }
    std::string kernel() const; // the kernel its work() launches (after start())
    uint64_t launches() const { return _launches; }

    // History loaded at start() instead of zeros: the ceil(ntaps / interp) - 1 RAW samples that
    // precede this block's first input (a time shard's halo); the block then reproduces the tail of a
    // longer stream, provided the shard starts at a multiple of D inputs.
    void set_initial_history(const std::vector<gr_complex>& h) { _state.set_initial(h); }

private:
    std::vector<float> _taps;
    int _interp, _decim;
    history_state _state;
    uint64_t _launches = 0;
};
} // namespace hip
} // namespace gr
