// blocks::rational_resampler_ccf: CPU restatement of GNU Radio's rational_resampler_ccf
// (interpolation I, decimation D, L real taps h): zero-stuff by I, filter, keep every D-th sample,
//   y[n] = sum_{k<L} h[k] u[nD - k],   u[jI] = x[j], u = 0 elsewhere
// (D = 1 is interp_fir_filter_ccf). I and D are used as given, not reduced by their gcd. Zero initial
// history. Plain scalar code straight from the definition in fp32, taps in ascending order: it
// defines the semantics and is the flowgraph comparator of hip::rational_resampler_ccf, not a
// baseline to tune. A gr::resamp_block: every work() takes n D inputs and makes n I outputs, so it
// starts at phase 0 and keeps only the last ceil(L / I) - 1 raw inputs. Tags as the decimating
// blocks have them (offsets are not rescaled).
#pragma once
#include <gnuradio/resamp_block.hpp>

namespace gr {
namespace blocks {
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
    bool start() override;
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    const std::vector<float>& taps() const { return _taps; }
    int interp() const { return _interp; }
    int decim() const { return _decim; }

private:
    std::vector<float> _taps;
    int _interp, _decim;
    std::vector<gr_complex> _ext; // [history (Q-1 raw samples) | current input]
};
} // namespace blocks
} // namespace gr
