// blocks::rotator_cc: CPU restatement of GNU Radio's rotator_cc, y[i] = x[i] exp(j phase_inc_rad n)
// for absolute stream sample n, on a 64-bit fixed-point phase: the frequency is
// inc = round(frac(t) 2^64) mod 2^64 turns per sample (t = phase_inc_rad / 2 pi) and the phase of
// sample n is (n inc) mod 2^64 turns in plain uint64 wrap-around arithmetic, so it neither depends
// on how the stream is cut into work() calls nor degrades with the stream position (GNU Radio's
// block multiplies a running phasor and renormalises it). Plain scalar code with a double sincos:
// this block defines the semantics and is the flowgraph comparator of hip::rotator_cc, not a
// baseline to tune. Absent from the reference.
#pragma once
#include <cmath>
#include <gnuradio/sync_block.hpp>
#include <stdexcept>

namespace gr {
namespace blocks {

// round(frac(t) 2^64) mod 2^64, exact from the double (ties to even); negative t wraps
inline uint64_t phase_inc_turns(double t)
{
    if (!std::isfinite(t)) throw std::invalid_argument("phase_inc_turns: the frequency must be finite");
    const double f = std::fmod(t, 1.0); // exact, sign of t
    const double r = std::nearbyint(std::ldexp(std::fabs(f), 64));
    const uint64_t u = r >= 18446744073709551616.0 ? 0 : (uint64_t)r;
    return f < 0 ? (uint64_t)0 - u : u;
}
// exp(j 2 pi p / 2^64) from the top 53 bits of the phase
inline void phase_sincos(uint64_t p, double& s, double& c)
{
    const double th = 2.0 * M_PI * std::ldexp((double)(p >> 11), -53);
    s = std::sin(th);
    c = std::cos(th);
}

class rotator_cc : public sync_block
{
public:
    using sptr = std::shared_ptr<rotator_cc>;
    static sptr make(double phase_inc_rad)
    {
        auto p = std::make_shared<rotator_cc>(phase_inc_rad);
        p->add_port(port<gr_complex>::make("in", port_direction_t::INPUT));
        p->add_port(port<gr_complex>::make("out", port_direction_t::OUTPUT));
        return p;
    }
    explicit rotator_cc(double phase_inc_rad) : sync_block("rotator_cc"), _inc(phase_inc_turns(phase_inc_rad / (2.0 * M_PI))) {}
    bool start() override;
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    uint64_t phase_inc() const { return _inc; }
    // Stream index of the first sample of a run (a time shard starts past 0); read by start().
    void set_first_index(uint64_t n) { _first = n; }

private:
    uint64_t _inc;
    uint64_t _first = 0, _index = 0;
};
} // namespace blocks
} // namespace gr
