// gr::hip::pfb_synthesizer_ccf -- M channels into one band: the critically sampled polyphase synthesis
// filterbank (an M-point inverse DFT across the channels of every item, then M branch FIRs of
// ceil(L / M) real fp32 taps) in one kernel launch per work() (nsh_pfb_synthesizer_ccf,
// k_pfb_synth<M>: every input is read from HBM once and every output written once, 16 B per output
// sample in all). Semantics of blocks::pfb_synthesizer_ccf, the counterpart of
// hip::pfb_channelizer_ccf; M a power of two in [2, 64], at most 1024 taps and 32 per branch; no gain
// of M (scale the taps by M for unity gain).
// A gr::resamp_block with I = M, D = 1 (input items of M samples, scalar output): the plan and two
// raw-history buffers of (ceil(L / M) - 1) M samples are created on the first start() on the partition
// thread, the history is zeroed (or loaded from set_initial_history) on every start().
//
// Measured (kernel times on 2^26 outputs, one MI355X): (M, taps) = (4, 31)
// 180 us, (4, 127) 238, (16, 127) 194, (64, 127) 210, (64, 511) 265: 1.07 to 1.59 times a copy of the
// same bytes, level with hip::pfb_channelizer_ccf (0.98 to 1.09 times), and 11 to 165 times faster than
// the M rational resamplers, M rotators and M - 1 adders that produce the same stream.
#pragma once
#include <gnuradio/blocklib/hip/fir_stream_state.hpp>
#include <gnuradio/resamp_block.hpp>

namespace gr {
namespace hip {
class pfb_synthesizer_ccf : public resamp_block
{
public:
    using sptr = std::shared_ptr<pfb_synthesizer_ccf>;
    static sptr make(int nchans, const std::vector<float>& taps)
    {
        auto p = std::make_shared<pfb_synthesizer_ccf>(nchans, taps);
        p->add_port(port<gr_complex>::make("in", port_direction_t::INPUT, { (size_t)nchans }));
        p->add_port(port<gr_complex>::make("out", port_direction_t::OUTPUT));
        return p;
    }
    pfb_synthesizer_ccf(int nchans, const std::vector<float>& taps);
    ~pfb_synthesizer_ccf() override;
    bool start() override;
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    int nchans() const { return _nchans; }
    const std::vector<float>& taps() const { return _taps; }
    std::string kernel() const; // the kernel its work() launches (after start())
    uint64_t launches() const { return _launches; }

    // History loaded at start() instead of zeros: the ceil(ntaps / nchans) - 1 RAW input items
    // ((Q-1) nchans samples) that precede this block's first item (a time shard's halo); the block
    // then reproduces the tail of a longer stream.
    void set_initial_history(const std::vector<gr_complex>& h) { _state.set_initial(h); }

private:
    std::vector<float> _taps;
    int _nchans;
    history_state _state;
    uint64_t _launches = 0;
};
} // namespace hip
} // namespace gr
