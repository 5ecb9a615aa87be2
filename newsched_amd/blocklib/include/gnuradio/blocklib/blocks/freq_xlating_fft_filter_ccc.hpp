// blocks::freq_xlating_fft_filter_ccc: CPU statement of GNU Radio's freq_xlating_fft_filter_ccc (tune
// to center_freq, filter with complex taps, decimate by a power of two up to 64). With
// f = center_freq / samp_rate and the 64-bit phase of rotator_cc.hpp at inc = phase_inc(-f):
//   y[m] = sum_{k<L} h[k] (x[mD - k] exp(j 2 pi phase(first_index + mD - k)))
// blocks::freq_xlating_fir_filter_ccf's definition with complex taps, in direct form: double sincos
// and double accumulation, zero initial history. It defines the semantics and is the flowgraph
// comparator of hip::freq_xlating_fft_filter_ccc (k_fft_xlat<N, D>, overlap-save on the GPU), not a
// baseline to tune. A gr::decim_block.
#pragma once
#include <gnuradio/blocklib/blocks/rotator_cc.hpp>
#include <gnuradio/decim_block.hpp>

namespace gr {
namespace blocks {
class freq_xlating_fft_filter_ccc : public decim_block
{
public:
    using sptr = std::shared_ptr<freq_xlating_fft_filter_ccc>;
    static sptr make(int decim, const std::vector<gr_complex>& taps, double center_freq, double samp_rate)
    {
        auto p = std::make_shared<freq_xlating_fft_filter_ccc>(decim, taps, center_freq, samp_rate);
        p->add_port(port<gr_complex>::make("in", port_direction_t::INPUT));
        p->add_port(port<gr_complex>::make("out", port_direction_t::OUTPUT));
        return p;
    }
    // throws std::invalid_argument for what nsh_fft_xlat_plan_create refuses: no taps or more than
    // 4096, a non-finite tap, a decimation that is no power of two in [1, 64], a samp_rate that is not
    // positive or a non-finite frequency
    freq_xlating_fft_filter_ccc(int decim, const std::vector<gr_complex>& taps, double center_freq, double samp_rate);
    bool start() override;
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    const std::vector<gr_complex>& taps() const { return _taps; }
    int decimation() const { return _decim; }
    uint64_t phase_inc() const { return _inc; }
    void set_first_index(uint64_t n) { _first = n; }

private:
    std::vector<gr_complex> _taps;
    int _decim;
    uint64_t _inc = 0;
    uint64_t _first = 0, _index = 0;
    std::vector<gr_complex> _ext; // [history (L-1 raw samples) | current input]
};
} // namespace blocks
} // namespace gr
