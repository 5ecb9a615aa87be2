// blocks::pfb_channelizer_ccf: CPU restatement of GNU Radio's critically sampled polyphase filterbank
// channelizer. nchans = M channels, L real taps h; output item m is the vector of M channels
//   y[m][c] = sum_{k<L} h[k] x[mM - k] exp(+j 2 pi c k / M)          (0 <= c < M)
// channel c being the band centred at +c/M cycles per sample, moved to DC, filtered by h and
// decimated by M (channel 0 is DC, channels above M/2 the negative frequencies: GNU Radio's order).
// Zero initial history. Plain scalar code straight from the definition in fp32, with the M phasors
// exp(j 2 pi i / M) as constants computed in double: it defines the semantics and is the flowgraph
// comparator of hip::pfb_channelizer_ccf, not a baseline to tune. A gr::decim_block with
// decimation M: scalar input items, output items of M samples (port dims {M}).
#pragma once
#include <gnuradio/decim_block.hpp>

namespace gr {
namespace blocks {
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
    bool start() override;
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    const std::vector<float>& taps() const { return _taps; }
    int nchans() const { return _nchans; }

private:
    std::vector<float> _taps;
    int _nchans;
    std::vector<gr_complex> _w;   // exp(j 2 pi i / M), i < M
    std::vector<gr_complex> _ext; // [history (L-1 raw samples) | current input]
};
} // namespace blocks
} // namespace gr
