// gr::hip::rotator_cc -- y[i] = x[i] exp(j phase_inc_rad n) on the device, n the absolute stream
// sample, on the 64-bit fixed-point phase of blocks::rotator_cc (same increment, so the two blocks
// agree to fp32 rounding at any stream position). One k_rotate launch per work() (nsh_rotate_cc),
// whatever the item count and the ring pointers' 8-byte alignment. The sample counter is reset by
// start() to set_first_index() (default 0) and advanced by the items consumed.
#pragma once
#include <gnuradio/blocklib/blocks/rotator_cc.hpp>
#include <gnuradio/sync_block.hpp>

namespace gr {
namespace hip {
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
    explicit rotator_cc(double phase_inc_rad)
        : sync_block("rotator_cc (hip)"), _inc(blocks::phase_inc_turns(phase_inc_rad / (2.0 * M_PI)))
    {
    }
    bool start() override
    {
        _index = _first;
        return sync_block::start();
    }
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override;
    uint64_t phase_inc() const { return _inc; }
    void set_first_index(uint64_t n) { _first = n; }
    uint64_t launches() const { return _launches; }

private:
    uint64_t _inc;
    uint64_t _first = 0, _index = 0;
    uint64_t _launches = 0;
};
} // namespace hip
} // namespace gr
