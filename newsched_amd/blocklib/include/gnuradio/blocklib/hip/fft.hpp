// gr::hip::fft_vcc (16 to 8192 points, a power of two; forward or inverse, unnormalised; an
// optional real window on the input and an optional half-frame shift, GNU Radio's conventions:
// include/nsh_hip.h, "FFT plan") and gr::hip::channelizer_vcc (fft -> multiply by w -> ifft at
// 1024 points, fused; BASELINE config C4).
// Items are vectors of fft_size complex samples (port dims {fft_size}, 8 fft_size bytes per item).
#pragma once
#include <gnuradio/sync_block.hpp>

namespace gr {
namespace hip {
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
    ~fft_vcc() override;
    bool start() override; // creates the plan on the current device
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    bool forward() const { return _forward; }
    size_t fft_size() const { return _fft_size; }
    const std::vector<float>& window() const { return _window; }
    bool shift() const { return _shift; }

private:
    size_t _fft_size;
    bool _forward, _shift;
    std::vector<float> _window;
    void* _plan = nullptr;
    int _plan_dev = -1;
};

class channelizer_vcc : public sync_block
{
public:
    using sptr = std::shared_ptr<channelizer_vcc>;
    static sptr make(const std::vector<gr_complex>& w)
    {
        auto p = std::make_shared<channelizer_vcc>(w);
        p->add_port(port<gr_complex>::make("in", port_direction_t::INPUT, { 1024 }));
        p->add_port(port<gr_complex>::make("out", port_direction_t::OUTPUT, { 1024 }));
        return p;
    }
    explicit channelizer_vcc(const std::vector<gr_complex>& w);
    const std::vector<gr_complex>& w() const { return _w; }
    ~channelizer_vcc() override;
    bool start() override;
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;

private:
    std::vector<gr_complex> _w;
    void* _wdev = nullptr;
};
} // namespace hip
} // namespace gr
