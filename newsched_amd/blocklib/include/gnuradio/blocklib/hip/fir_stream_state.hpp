// State shared by the gr::hip blocks whose kernels carry an input history from one work() call to
// the next (fir_filter_ccf, fir_filter_cascade_ccf, freq_xlating_fir_filter_ccf,
// pfb_channelizer_ccf, pfb_synthesizer_ccf, the resamplers), because the block API has no history (reference
// runtime/include/gnuradio/sync_block.hpp:36-86):
//   history_state  the libnsh_hip plan and the two history buffers a block ping-pongs between calls
//   event_pool     the (start, stop) HIP event pairs of a block's timed launches
// Both are members of their block; every message they throw names it. Implemented in blocks_hip.cpp.
#pragma once
#include <gnuradio/types.hpp>

#include <cstdint>
#include <functional>
#include <string>
#include <utility>
#include <vector>

namespace gr {
namespace hip {

class history_state
{
public:
    using destroy_fn = int (*)(void*);
    // make_plan(dev, &plan) creates the block's plan on dev, throwing when it cannot, and returns
    // the history length in samples
    using plan_factory = std::function<size_t(int, void**)>;

    history_state(const char* who, destroy_fn destroy) : _who(who), _destroy(destroy) {}
    ~history_state() { release(); }
    history_state(const history_state&) = delete;
    history_state& operator=(const history_state&) = delete;

    // History loaded by begin_run() instead of zeros: the samples that precede the first input.
    void set_initial(const std::vector<gr_complex>& h) { _init = h; }
    bool has_initial() const { return !_init.empty(); }

    // Device state lives on the device of the thread that runs the block: true when it was made
    // on another one than dev (prepare() then makes it anew).
    bool on_other_device(int dev) const { return _plan && dev != _dev; }
    // The plan and the two buffers on dev: made by the first call and after a device change.
    void prepare(int dev, const plan_factory& make_plan);
    // A fresh stream: the first call reads a null history (zeros in the kernel, no memset launch;
    // every call writes its hist_out in full, so the buffers need no clearing), or the initial
    // history, which must have the plan's history length.
    void begin_run(void* stream);

    void* plan() const { return _plan; }
    const float* hist_in() const { return _zero ? nullptr : (const float*)_hist[_cur]; }
    float* hist_out() const { return (float*)_hist[_cur ^ 1]; }
    void flip() // after a call: what it wrote is the next one's history
    {
        _zero = false;
        _cur ^= 1;
    }
    void release();

private:
    const std::string _who;
    const destroy_fn _destroy;
    std::vector<gr_complex> _init;
    int _dev = -1;
    void* _plan = nullptr;
    size_t _len = 0; // history samples
    void* _hist[2] = { nullptr, nullptr };
    bool _zero = true; // the next call reads a null history (zeros): set by begin_run()
    int _cur = 0;
};

// Kernel timing: a timed launch records its own start / stop events (nsh_time_next_launch) unless
// NSH_FIR_TIMING=records asks for the two event records around the call (A/B of the two forms).
// Pairs are reused: the pool grows only when more launches are pending than ever before.
class event_pool
{
public:
    explicit event_pool(const char* who) : _what(std::string(who) + " timing") {}
    ~event_pool() { release(); }
    event_pool(const event_pool&) = delete;
    event_pool& operator=(const event_pool&) = delete;

    void arm(void* stream);      // before the launch to be timed: takes the next pair
    void recorded(void* stream); // after it
    size_t pending() const { return _used; }
    // total + the kernel times (ms) of the pending pairs, in launch order; waits for each
    double sum_ms(double total = 0);
    void reuse() { _used = 0; } // the pending pairs are free again
    void release();

private:
    const std::string _what;
    std::vector<std::pair<void*, void*>> _ev; // (start, stop) per launch
    size_t _used = 0;
};

} // namespace hip
} // namespace gr
