// gr::hip::freq_xlating_fft_filter_ccc -- tune to center_freq, filter with complex taps (1 to 4096),
// decimate by D in {1, 2, 4, 8, 16, 32, 64} by overlap-save, GNU Radio's freq_xlating_fft_filter_ccc,
// one kernel launch per work() (nsh_fft_xlat_ccc, k_fft_xlat<N, D>: window -> FFT of N -> times the
// band-pass taps' spectrum -> fold to N/D bins -> inverse FFT of N/D -> rotate -> valid part).
// Semantics of blocks::freq_xlating_fft_filter_ccc (64-bit phase, a signal at +center_freq lands at
// DC). gr::hip::freq_xlating_fft_filter_ccf is the same block for real taps. fft_size is 1024, 2048,
// 4096 or 8192 with ntaps <= fft_size / 2, or 0: hip::fft_filter_ccc's rule.
// A gr::decim_block like hip::freq_xlating_fir_filter_ccf: the plan and two (ntaps-1)-sample
// raw-history buffers are created on the first start() on the partition thread, the history is
// zeroed (or loaded from set_initial_history) and the sample counter reset to set_first_index() on
// every start(). Accuracy (include/nsh_hip.h): |y - y_ref| <= 1e-5 |y_ref| + 1e-6 max|x in the
// frame's window| sum|h|; an output's rounding depends on its frame, and so on how the scheduler
// cuts the stream into work() calls: two runs of one flowgraph agree to that bound, not bit for bit.
// The phase is exact however the stream is cut.
//
// When to prefer it (kernel times per 2^26 inputs on one MI355X, real low-pass
// taps, profiles/fft_xlat_bench.json). Over hip::freq_xlating_fir_filter_ccf: at 127 taps for every
// D up to 16 (229 / 257 / 220 / 208 / 205 us at D = 1 / 2 / 4 / 8 / 16 against 809 / 454 / 406 / 251 /
// 221) and at (D, taps) = (16, 255) (236 against 283); not at D = 64, where the fused FIR is faster at
// 127 taps (164 us against 204) and level at 1024 (286 against 295). It is the only one of the two for
// complex taps or more than 1024. Over hip::rotator_cc -> hip::fir_filter_ccf(decim): at 127 and 255
// taps for every D the pair takes (0.64 to 0.82 of the pair's 286 to 355 us); not for long real taps,
// where the pair's polyphase-FFT FIR wins: 402 us against 444 at (8, 2048), 379 against 566 at
// (16, 4096). Against hip::fft_filter_ccc followed by a decimator it costs 0.94 to 1.17 of the
// undecimated filter alone (1.04 at D = 1) and writes 1/D of the bytes. It takes powers of two only,
// where the fused FIR takes any D in [1, 64].
#pragma once
#include <gnuradio/blocklib/hip/fir_stream_state.hpp>
#include <gnuradio/decim_block.hpp>

namespace gr {
namespace hip {
class freq_xlating_fft_filter_ccc : public decim_block
{
public:
    using sptr = std::shared_ptr<freq_xlating_fft_filter_ccc>;
    static sptr make(int decim, const std::vector<gr_complex>& taps, double center_freq, double samp_rate, size_t fft_size = 0)
    {
        auto p = std::make_shared<freq_xlating_fft_filter_ccc>(decim, taps, center_freq, samp_rate, fft_size);
        p->add_port(port<gr_complex>::make("in", port_direction_t::INPUT));
        p->add_port(port<gr_complex>::make("out", port_direction_t::OUTPUT));
        return p;
    }
    // throws std::invalid_argument for what nsh_fft_xlat_plan_create refuses: no taps or more than
    // 4096, a non-finite tap, a decimation that is no power of two in [1, 64], a samp_rate that is not
    // positive or a non-finite frequency, an fft_size other than 0, 1024, 2048, 4096, 8192,
    // ntaps > fft_size / 2
    freq_xlating_fft_filter_ccc(int decim, const std::vector<gr_complex>& taps, double center_freq, double samp_rate,
                                size_t fft_size = 0, const char* name = "freq_xlating_fft_filter_ccc (hip)");
    ~freq_xlating_fft_filter_ccc() override;
    bool start() override;
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    int decimation() const { return _decim; }
    const std::vector<gr_complex>& taps() const { return _taps; }
    size_t fft_size() const;    // the frame size in use (after start(); before it, the argument)
    uint64_t phase_inc() const; // phase_inc(-center_freq / samp_rate) (after start())
    std::string kernel() const; // the kernel its work() launches (after start())
    uint64_t launches() const { return _launches; }

    // History loaded at start() instead of zeros: the ntaps-1 RAW samples that precede this block's
    // first input (a time shard's halo); with set_first_index the block reproduces the tail of a
    // longer stream.
    void set_initial_history(const std::vector<gr_complex>& h) { _state.set_initial(h); }
    void set_first_index(uint64_t n) { _first = n; }

private:
    std::vector<gr_complex> _taps;
    int _decim;
    double _freq_norm = 0;
    size_t _fft_size;
    history_state _state;
    uint64_t _first = 0, _index = 0;
    uint64_t _launches = 0;
};

class freq_xlating_fft_filter_ccf : public freq_xlating_fft_filter_ccc
{
public:
    using sptr = std::shared_ptr<freq_xlating_fft_filter_ccf>;
    static sptr make(int decim, const std::vector<float>& taps, double center_freq, double samp_rate, size_t fft_size = 0)
    {
        auto p = std::make_shared<freq_xlating_fft_filter_ccf>(decim, taps, center_freq, samp_rate, fft_size);
        p->add_port(port<gr_complex>::make("in", port_direction_t::INPUT));
        p->add_port(port<gr_complex>::make("out", port_direction_t::OUTPUT));
        return p;
    }
    freq_xlating_fft_filter_ccf(int decim, const std::vector<float>& taps, double center_freq, double samp_rate,
                                size_t fft_size = 0)
        : freq_xlating_fft_filter_ccc(decim, std::vector<gr_complex>(taps.begin(), taps.end()), center_freq, samp_rate, fft_size,
                                      "freq_xlating_fft_filter_ccf (hip)")
    {
    }
};
} // namespace hip
} // namespace gr
