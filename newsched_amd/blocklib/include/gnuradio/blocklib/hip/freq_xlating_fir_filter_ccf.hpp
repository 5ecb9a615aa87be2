// gr::hip::freq_xlating_fir_filter_ccf -- tune to center_freq, low-pass (real fp32 taps), decimate
// by any D in [1, 64], in one fused kernel launch per work() (nsh_fir_xlat_ccf, k_fir_xlat<R,S>:
// the input is read from HBM once, rotated at staging, filtered in fp32 direct form). Semantics of
// blocks::freq_xlating_fir_filter_ccf (64-bit phase, a signal at +center_freq lands at DC).
// A gr::decim_block like hip::fir_filter_ccf: the plan and two (ntaps-1)-sample raw-history buffers
// are created on the first start() on the partition thread, the history is zeroed (or loaded from
// set_initial_history) and the sample counter reset to set_first_index() on every start().
//
// When to chain hip::rotator_cc -> hip::fir_filter_ccf instead (measured at
// 127 taps on 2^26 inputs): the fused kernel wins at decimation 8 (0.88x the staged pair's time) and
// 16 (0.83x); at D = 1, 2 and 4 the staged pair is faster (2.5x, 1.6x, 1.5x), because there the MFMA
// FIR does the arithmetic this kernel does on the vector ALUs. At D = 16 with 255 taps the two are
// level (1.04x), and the staged pair is limited to decimation 1, 2, 4, 8 and 16.
//
// When to prefer hip::freq_xlating_fft_filter_ccf instead (the same 127 taps
// and 2^26 inputs, kernel times of one run): at every power-of-two decimation up to 16 the
// overlap-save block is faster than this one, 229 / 257 / 220 / 208 / 205 us at D = 1 / 2 / 4 / 8 / 16
// against 809 / 454 / 406 / 251 / 221 us here, and than the staged pair at each of them (355 / 312 /
// 292 / 309 / 286 us); at (D, taps) = (16, 255) it takes 236 us against 283 here. This block stays
// the faster one at D = 64 (164 us against 204 at 127 taps; level, 286 against 295, at 1024 taps) and
// the only one for a decimation that is no power of two.
#pragma once
#include <gnuradio/blocklib/hip/fir_stream_state.hpp>
#include <gnuradio/decim_block.hpp>

namespace gr {
namespace hip {
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
    ~freq_xlating_fir_filter_ccf() override;
    bool start() override;
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    int decimation() const { return _decim; }
    const std::vector<float>& taps() const { return _taps; }
    uint64_t phase_inc() const;  // phase_inc(-center_freq / samp_rate) (after start())
    std::string kernel() const;  // the kernel its work() launches (after start())
    uint64_t launches() const { return _launches; }

    // History loaded at start() instead of zeros: the ntaps-1 RAW samples that precede this block's
    // first input (a time shard's halo); with set_first_index the block reproduces the tail of a
    // longer stream.
    void set_initial_history(const std::vector<gr_complex>& h) { _state.set_initial(h); }
    void set_first_index(uint64_t n) { _first = n; }

private:
    std::vector<float> _taps;
    int _decim;
    double _freq_norm;
    history_state _state;
    uint64_t _first = 0, _index = 0;
    uint64_t _launches = 0;
};
} // namespace hip
} // namespace gr
