// gr::hip::psd_vcf -- the spectrum estimate fft_vcc -> complex_to_mag_squared -> integrate_ff
// (-> nlog10_ff) in one pass over the input (nsh_psd_cf, k_psd<N, LIN>: windowed FFT, |X|^2 and the
// sum over navg frames in registers; 8 + 4 / navg bytes of HBM traffic per sample). Semantics:
// blocks/psd.hpp and include/nsh_hip.h, "psd_vcf". Items in are vectors of fft_size complex samples
// (port dims {fft_size}), items out vectors of fft_size floats, one per navg input vectors: a
// gr::decim_block of decimation navg, so work() consumes whole groups of navg vectors only.
// The plan is created in start() on the current device. A vector's value does not depend on how the
// scheduler cuts the stream into work() calls: two runs of one flowgraph agree bit for bit.
// Frames do not overlap; Welch overlap and exponential averaging are not provided.
#pragma once
#include <gnuradio/blocklib/hip/fir_stream_state.hpp>
#include <gnuradio/decim_block.hpp>

namespace gr {
namespace hip {
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
    // throws std::invalid_argument for what nsh_psd_plan_create refuses, in its order: fft_size not a
    // power of two in [16, 8192]; navg outside [1, 65536]; a window whose length is not fft_size
    // (empty: none) or with a non-finite entry; a scale that is not finite or negative (0: 1 / navg)
    psd_vcf(size_t fft_size, size_t navg, const std::vector<float>& window = {}, bool shift = false, float scale = 0,
            bool db = false);
    ~psd_vcf() override;
    bool start() override; // creates the plan on the current device
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    size_t fft_size() const { return _fft_size; }
    size_t navg() const { return _navg; }
    const std::vector<float>& window() const { return _window; }
    bool shift() const { return _shift; }
    float scale() const { return _scale; } // the factor in use
    bool db() const { return _db; }
    std::string kernel() const; // the kernel its work() launches (after start())
    uint64_t launches() const { return _launches; }

    // Per-call kernel timing with HIP events on the launch stream, as fft_filter_ccc's.
    void enable_timing(bool on) { _timing = on; }
    double kernel_ms();
    uint64_t timed_vectors() const { return _timed_vectors; }

private:
    size_t _fft_size, _navg;
    bool _shift, _db;
    float _scale;
    std::vector<float> _window;
    void* _plan = nullptr;
    int _plan_dev = -1;
    event_pool _ev;
    bool _timing = false;
    uint64_t _launches = 0, _timed_vectors = 0;
};
} // namespace hip
} // namespace gr
