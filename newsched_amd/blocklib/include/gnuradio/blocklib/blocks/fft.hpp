// blocks::fft_vcc: complex FFT of fft_size = 2^k points, 16 <= fft_size <= 8192, forward or inverse,
// unnormalised both ways, with an optional real window on the input and an optional half-frame
// shift (GNU Radio's fft_vcc conventions). With w[n] = 1 without a window:
//   forward  X[k] = sum_n x[n] w[n] e^{-2 pi i kn/N};  shift: out[k] = X[(k + N/2) mod N]
//   inverse  y[n] = x[n] w[n] (the window indexed by the input position as it arrives);
//            shift: y'[n] = y[(n + N/2) mod N];  out[m] = sum_n y'[n] e^{+2 pi i mn/N}
// The window product is one fp32 multiply per component; the transform is a plain radix-2 in
// double with twiddles from cos / sin in double, rounded to float once. It defines the semantics
// and is the flowgraph comparator and CPU path of hip::fft_vcc, not a baseline to tune.
// Items are vectors of fft_size complex samples (port dims {fft_size}).
#pragma once
#include <gnuradio/sync_block.hpp>

#include <complex>

namespace gr {
namespace blocks {
class fft_vcc : public sync_block
{
public:
    using sptr = std::shared_ptr<fft_vcc>;
    static sptr make(size_t fft_size = 1024, bool forward = true, const std::vector<float>& window = {}, bool shift = false)
    {
        auto p = std::make_shared<fft_vcc>(fft_size, forward, window, shift);
        p->add_port(port<gr_complex>::make("in", port_direction_t::INPUT, { fft_size }));
        p->add_port(port<gr_complex>::make("out", port_direction_t::OUTPUT, { fft_size }));
        return p;
    }
    // throws std::invalid_argument: fft_size not a power of two in [16, 8192], a window whose
    // length is not fft_size (empty: none)
    fft_vcc(size_t fft_size, bool forward, const std::vector<float>& window = {}, bool shift = false);
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    bool forward() const { return _forward; }
    size_t fft_size() const { return _fft_size; }
    const std::vector<float>& window() const { return _window; }
    bool shift() const { return _shift; }

private:
    size_t _fft_size;
    bool _forward, _shift;
    std::vector<float> _window;
    std::vector<std::complex<double>> _tw, _a; // e^{-+2 pi i t / N}, t < N / 2; the frame in work
};
} // namespace blocks
} // namespace gr
