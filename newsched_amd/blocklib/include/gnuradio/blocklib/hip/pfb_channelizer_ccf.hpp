// gr::hip::pfb_channelizer_ccf -- all M channels of a band at once: the critically sampled
// polyphase filterbank (M branch FIRs of ceil(L / M) real fp32 taps, then an M-point inverse DFT) in
// one kernel launch per work() (nsh_pfb_channelizer_ccf, k_pfb<M>: the input is read from HBM once,
// 16 B per input sample in all). Semantics of blocks::pfb_channelizer_ccf; M a power of two in
// [2, 64], at most 1024 taps and 32 per branch. Channel c of every output item equals
// hip::freq_xlating_fir_filter_ccf(M, taps, c / M, 1.0) on the same stream, to fp32 rounding
// relative to the loudest channel.
// A gr::decim_block with decimation M like hip::freq_xlating_fir_filter_ccf: the plan and two
// (ntaps-1)-sample raw-history buffers are created on the first start() on the partition thread, the
// history is zeroed (or loaded from set_initial_history) on every start().
//
// Against the M hip::freq_xlating_fir_filter_ccf blocks that produce the same channels (DESIGN.md
// section 4.4, kernel times on 2^26 inputs, one MI355X): (M, taps) = (4, 31) 182 us against 1061 us,
// (4, 127) 231 against 1661, (16, 127) 193 against 3582, (64, 511) 241 against 13868, (64, 127) 202
// against 10627: 5.8 to 57 times faster, at 56 to 74 % of the HBM bound on 16 B per input sample
// (1.1 to 1.5 times the time of a copy of the same bytes).
#pragma once
#include <gnuradio/blocklib/hip/fir_stream_state.hpp>
#include <gnuradio/decim_block.hpp>

namespace gr {
namespace hip {
class pfb_channelizer_ccf : public decim_block
{
public:
    using sptr = std::shared_ptr<pfb_channelizer_ccf>;
    static sptr make(int nchans, const std::vector<float>& taps)
    {
        auto p = std::make_shared<pfb_channelizer_ccf>(nchans, taps);
        p->add_port(port<gr_complex>::make("in", port_direction_t::INPUT));
        p->add_port(port<gr_complex>::make("out", port_direction_t::OUTPUT, { (size_t)nchans }));
        return p;
    }
    pfb_channelizer_ccf(int nchans, const std::vector<float>& taps);
    ~pfb_channelizer_ccf() override;
    bool start() override;
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    int nchans() const { return _nchans; }
    const std::vector<float>& taps() const { return _taps; }
    std::string kernel() const; // the kernel its work() launches (after start())
    uint64_t launches() const { return _launches; }

    // History loaded at start() instead of zeros: the ntaps-1 RAW samples that precede this block's
    // first input (a time shard's halo); the block then reproduces the tail of a longer stream.
    void set_initial_history(const std::vector<gr_complex>& h) { _state.set_initial(h); }

private:
    std::vector<float> _taps;
    int _nchans;
    history_state _state;
    uint64_t _launches = 0;
};
} // namespace hip
} // namespace gr
