// gr::hip::fft_filter_ccc -- FIR filter with complex taps (1 to 4096) at decimation 1 by overlap-save,
// GNU Radio's fft_filter_ccc: y[n] = sum_k h[k] x[n-k], one kernel launch per work()
// (nsh_fft_filter_ccc, k_fft_xlat<N, 1, false>: window -> FFT -> times the taps' spectrum -> inverse FFT ->
// valid part; about 16 B of HBM traffic per output whatever the tap count). gr::hip::fft_filter_ccf
// is the same block for real taps (zero imaginary parts). fft_size is 1024, 2048, 4096 or 8192 with
// ntaps <= fft_size / 2, or 0: 1024 up to 256 taps, 2048 up to 512, 4096 up to 2048, 8192 above.
// A gr::sync_block: the plan and two (ntaps-1)-sample raw-history buffers are created on the first
// start() on the partition thread, the history is zeroed (or loaded from set_initial_history) on every
// start(). Accuracy (include/nsh_hip.h): |y - y_ref| <= 1e-5 |y_ref| + 1e-6 max|x in the frame's
// window| sum|h|; an output's rounding depends on its frame, and so on how the scheduler cuts the
// stream into work() calls: two runs of one flowgraph agree to that bound, not bit for bit.
//
// When to prefer hip::fft_filter_ccf over hip::fir_filter_ccf on real taps at decimation 1: from 162
// taps on. Up to 161 taps fir_filter_ccf(AUTO) runs its MFMA kernel (181 us per 2^26 samples at 127 and
// at 161 taps, against 220 and 228 us here); from 162 on it runs the fp32 direct form, 5.6 ms at 162
// taps, 33 ms at 1024 and 132 ms at 4096, where this block takes 219, 340 and 726 us (DESIGN.md
// section 4.8, kernel times, one MI355X).
#pragma once
#include <gnuradio/blocklib/hip/fir_stream_state.hpp>
#include <gnuradio/sync_block.hpp>

namespace gr {
namespace hip {
class fft_filter_ccc : public sync_block
{
public:
    using sptr = std::shared_ptr<fft_filter_ccc>;
    static sptr make(const std::vector<gr_complex>& taps, size_t fft_size = 0)
    {
        auto p = std::make_shared<fft_filter_ccc>(taps, fft_size);
        p->add_port(port<gr_complex>::make("in", port_direction_t::INPUT));
        p->add_port(port<gr_complex>::make("out", port_direction_t::OUTPUT));
        return p;
    }
    // throws std::invalid_argument for what nsh_fft_filter_plan_create refuses: no taps or more than
    // 4096, a non-finite tap, an fft_size other than 0, 1024, 2048, 4096, 8192, ntaps > fft_size / 2
    fft_filter_ccc(const std::vector<gr_complex>& taps, size_t fft_size = 0, const char* name = "fft_filter_ccc (hip)");
    ~fft_filter_ccc() override;
    bool start() override;
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    const std::vector<gr_complex>& taps() const { return _taps; }
    size_t fft_size() const;    // the frame size in use (after start(); before it, the argument)
    std::string kernel() const; // the kernel its work() launches (after start())
    uint64_t launches() const { return _launches; }

    // History loaded at start() instead of zeros: the ntaps-1 RAW samples that precede this block's
    // first input (a time shard's halo).
    void set_initial_history(const std::vector<gr_complex>& h) { _state.set_initial(h); }

    // Per-launch kernel timing with HIP events on the launch stream, as fir_filter_cascade_ccf's.
    void enable_timing(bool on) { _timing = on; }
    double kernel_ms();
    uint64_t timed_samples() const { return _timed_samples; }

private:
    std::vector<gr_complex> _taps;
    size_t _fft_size;
    history_state _state;
    event_pool _ev;
    bool _timing = false;
    uint64_t _launches = 0, _timed_samples = 0;
};

class fft_filter_ccf : public fft_filter_ccc
{
public:
    using sptr = std::shared_ptr<fft_filter_ccf>;
    static sptr make(const std::vector<float>& taps, size_t fft_size = 0)
    {
        auto p = std::make_shared<fft_filter_ccf>(taps, fft_size);
        p->add_port(port<gr_complex>::make("in", port_direction_t::INPUT));
        p->add_port(port<gr_complex>::make("out", port_direction_t::OUTPUT));
        return p;
    }
    fft_filter_ccf(const std::vector<float>& taps, size_t fft_size = 0)
        : fft_filter_ccc(std::vector<gr_complex>(taps.begin(), taps.end()), fft_size, "fft_filter_ccf (hip)")
    {
    }
};
} // namespace hip
} // namespace gr
