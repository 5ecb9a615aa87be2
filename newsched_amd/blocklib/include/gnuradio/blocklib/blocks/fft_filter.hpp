// blocks::fft_filter_ccc: CPU statement of GNU Radio's fft_filter_ccc at decimation 1 (complex
// stream, complex taps), y[n] = sum_k h[k] x[n-k], zero initial history. It defines the semantics
// that hip::fft_filter_ccc (k_fft_xlat<N, 1, false>, overlap-save on the GPU) is tested against, and computes
// them in the plain direct form, accumulated in double and rounded once per output: no frames, so its
// output does not depend on how the stream is cut into work() calls. A gr::sync_block.
// For real taps on the GPU, prefer hip::fft_filter_ccf to hip::fir_filter_ccf from 162 taps on (where
// fir_filter_ccf(AUTO) leaves its MFMA kernel for the fp32 direct form: 5.6 ms against 219 us per 2^26
// samples at 162 taps).
#pragma once
#include <gnuradio/sync_block.hpp>

namespace gr {
namespace blocks {
class fft_filter_ccc : public sync_block
{
public:
    using sptr = std::shared_ptr<fft_filter_ccc>;
    static sptr make(const std::vector<gr_complex>& taps)
    {
        auto p = std::make_shared<fft_filter_ccc>(taps);
        p->add_port(port<gr_complex>::make("in", port_direction_t::INPUT));
        p->add_port(port<gr_complex>::make("out", port_direction_t::OUTPUT));
        return p;
    }
    // throws std::invalid_argument: no taps, more than 4096, a non-finite tap
    explicit fft_filter_ccc(const std::vector<gr_complex>& taps);
    bool start() override; // zero history
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    const std::vector<gr_complex>& taps() const { return _taps; }

private:
    std::vector<gr_complex> _taps;
    std::vector<gr_complex> _ext; // [history (L-1) | current input]
};
} // namespace blocks
} // namespace gr
