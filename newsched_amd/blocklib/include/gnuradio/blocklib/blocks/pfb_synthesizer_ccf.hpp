// blocks::pfb_synthesizer_ccf: the critically sampled polyphase synthesis filterbank, the exact
// counterpart of blocks::pfb_channelizer_ccf. nchans = M channels, L real taps h; input item m is the
// vector X[m][c] of the M channels (what the channelizer emits), the output a stream at M times the
// item rate:
//   y[n] = sum_{c<M} sum_{m'} X[m'][c] h[n - m' M] exp(+j 2 pi c n / M)          0 <= n - m' M < L
// each channel zero-stuffed by M, filtered by h (used as given: no gain of M), moved to +c/M cycles
// per sample, and the M results summed. Channel 0 is DC, channels above M/2 the negative frequencies.
// Not GNU Radio's block of the name (M separate streams, a 2x mode, a channel map). Zero initial
// history. Plain scalar fp32 code in polyphase form (an M-point sum per output branch with the M
// phasors exp(j 2 pi i / M) as constants computed in double, then the branch's taps in ascending
// order): it defines the semantics and is the flowgraph comparator of hip::pfb_synthesizer_ccf, not a
// baseline to tune. A gr::resamp_block with I = M, D = 1: input items of M samples (port dims {M}),
// scalar output items.
#pragma once
#include <gnuradio/resamp_block.hpp>

namespace gr {
namespace blocks {
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
    bool start() override;
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    const std::vector<float>& taps() const { return _taps; }
    int nchans() const { return _nchans; }

private:
    std::vector<float> _taps;
    int _nchans;
    std::vector<gr_complex> _w;   // exp(j 2 pi i / M), i < M
    std::vector<gr_complex> _ext; // [history (Q-1 raw items) | current input]
    std::vector<gr_complex> _v;   // the items of _ext, transformed
};
} // namespace blocks
} // namespace gr
