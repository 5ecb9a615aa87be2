// blocks::psd_vcf: the spectrum estimate fft_vcc -> complex_to_mag_squared -> integrate_ff
// (-> nlog10_ff) as one block. Items in are vectors of fft_size complex samples, items out vectors
// of fft_size floats, one per navg input vectors (a decim_block of decimation navg). With N =
// fft_size, K = navg, w[n] = 1 without a window, output vector j from input vectors jK .. jK+K-1:
//   X_f[k]   = sum_n x_f[n] w[n] e^{-2 pi i kn/N}
//   P_j[k]   = scale sum_f |X_f[k]|^2                    scale 0: 1 / navg
//   out_j[k] = P_j[k ^ (shift ? N/2 : 0)],  or 10 log10 of it (db; a zero sum gives -inf)
// Frames do not overlap. The window product is one fp32 multiply per component; transform, squares,
// sum, scale and logarithm are computed in double and rounded to float once. It defines the
// semantics and is the flowgraph comparator and CPU path of hip::psd_vcf, not a baseline to tune.
#pragma once
#include <gnuradio/decim_block.hpp>

#include <complex>

namespace gr {
namespace blocks {
class psd_vcf : public decim_block
{
public:
    using sptr = std::shared_ptr<psd_vcf>;
    static sptr make(size_t fft_size, size_t navg, const std::vector<float>& window = {}, bool shift = false, float scale = 0,
                     bool db = false)
    {
        auto p = std::make_shared<psd_vcf>(fft_size, navg, window, shift, scale, db);
        p->add_port(port<gr_complex>::make("in", port_direction_t::INPUT, { fft_size }));
        p->add_port(port<float>::make("out", port_direction_t::OUTPUT, { fft_size }));
        return p;
    }
    // throws std::invalid_argument, in this order: fft_size not a power of two in [16, 8192]; navg
    // outside [1, 65536]; a window whose length is not fft_size (empty: none) or with a non-finite
    // entry; a scale that is not finite or negative (0: 1 / navg)
    psd_vcf(size_t fft_size, size_t navg, const std::vector<float>& window = {}, bool shift = false, float scale = 0,
            bool db = false);
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    size_t fft_size() const { return _fft_size; }
    size_t navg() const { return _navg; }
    const std::vector<float>& window() const { return _window; }
    bool shift() const { return _shift; }
    float scale() const { return _scale; } // the factor in use
    bool db() const { return _db; }

private:
    size_t _fft_size, _navg;
    bool _shift, _db;
    float _scale;
    std::vector<float> _window;
    std::vector<std::complex<double>> _tw, _a; // e^{-2 pi i t / N}, t < N / 2; the frame in work
    std::vector<double> _sum;
};
} // namespace blocks
} // namespace gr
