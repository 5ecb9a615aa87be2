// blocks::freq_xlating_fir_filter_ccf: CPU restatement of GNU Radio's block of that name (tune to
// center_freq, low-pass with real taps, decimate). With f = center_freq / samp_rate and the 64-bit
// phase of rotator_cc.hpp at inc = phase_inc(-f):
//   y[m] = sum_{k<L} h[k] (x[mD - k] exp(j 2 pi phase(first_index + mD - k)))
// which equals GNU Radio's e^{-j theta D m} sum_k h[k] e^{j theta k} x[mD - k], theta = 2 pi f: a
// signal at +center_freq lands at DC. Zero initial history. Plain scalar code, double sincos and
// double accumulation: it defines the semantics and is the flowgraph comparator of
// hip::freq_xlating_fir_filter_ccf, not a baseline to tune. A gr::decim_block.
#pragma once
#include <gnuradio/blocklib/blocks/rotator_cc.hpp>
#include <gnuradio/decim_block.hpp>

namespace gr {
namespace blocks {
class freq_xlating_fir_filter_ccf : public decim_block
{
public:
    using sptr = std::shared_ptr<freq_xlating_fir_filter_ccf>;
    static sptr make(int decim, const std::vector<float>& taps, double center_freq, double samp_rate)
    {
        auto p = std::make_shared<freq_xlating_fir_filter_ccf>(decim, taps, center_freq, samp_rate);
        p->add_port(port<gr_complex>::make("in", port_direction_t::INPUT));
        p->add_port(port<gr_complex>::make("out", port_direction_t::OUTPUT));
        return p;
    }
    freq_xlating_fir_filter_ccf(int decim, const std::vector<float>& taps, double center_freq, double samp_rate);
    bool start() override;
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    const std::vector<float>& taps() const { return _taps; }
    int decimation() const { return _decim; }
    uint64_t phase_inc() const { return _inc; }
    void set_first_index(uint64_t n) { _first = n; }

private:
    std::vector<float> _taps;
    int _decim;
    uint64_t _inc;
    uint64_t _first = 0, _index = 0;
    std::vector<gr_complex> _ext; // [history (L-1 raw samples) | current input]
};
} // namespace blocks
} // namespace gr
