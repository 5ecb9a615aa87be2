// I:D block, the rate-changing sibling of decim_block: every call handles n units of D items per
// input and I items per output. n is clamped to the smallest count such that D items per unit are
// readable on every input and I items per unit writable on every output; work() sees n * D inputs
// and n * I outputs and sets n_produced (the same multiple of I on all outputs); every input then
// consumes (n_produced / I) * D. No unit readable: WORK_INSUFFICIENT_INPUT_ITEMS; a unit readable but
// no room for its I outputs: WORK_INSUFFICIENT_OUTPUT_ITEMS (graph_executor then waits for the
// reader; a block of this kind can meet 1 .. I-1 free items, which no other block can). Leftover input shorter than D at the end of a stream is dropped,
// as the decimators drop theirs. Buffer managers give the edge into such a block at least 2 * D
// items and the edge out of it at least 2 * I (schedulers/lib/buffer_management.cpp).
#pragma once
#include <algorithm>
#include <gnuradio/block.hpp>
#include <limits>
#include <stdexcept>

namespace gr {

class resamp_block : public block
{
public:
    resamp_block(const std::string& name, unsigned interpolation, unsigned decimation)
        : block(name), _interp(interpolation ? interpolation : 1), _decim(decimation ? decimation : 1)
    {
    }
    unsigned interpolation() const { return _interp; }
    unsigned decimation() const { return _decim; }
    double relative_rate() const override { return (double)_interp / (double)_decim; }

    work_return_code_t do_work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override
    {
        int n = std::numeric_limits<int>::max(), n_room = n;
        for (auto& w : in) n = std::min(n, w.n_items / (int)_decim);
        for (auto& w : out) n_room = std::min(n_room, w.n_items / (int)_interp);
        if (n <= 0) return work_return_code_t::WORK_INSUFFICIENT_INPUT_ITEMS;
        // a unit is readable but fewer than I items are writable: the executor waits for the reader
        // (as missing input this would end the block at the end of the stream with items unread)
        if (n_room <= 0) return work_return_code_t::WORK_INSUFFICIENT_OUTPUT_ITEMS;
        n = std::min(n, n_room);
        for (auto& w : in) w.n_items = n * (int)_decim;
        for (auto& w : out) w.n_items = n * (int)_interp;

        const work_return_code_t ret = work(in, out);

        int produced = -1;
        for (size_t i = 0; i < out.size(); ++i) {
            if (i == 0)
                produced = out[i].n_produced;
            else if (out[i].n_produced != produced)
                throw std::runtime_error("outputs for resamp_block must produce same number of items");
        }
        if (produced > 0 && produced % (int)_interp)
            throw std::runtime_error("outputs for resamp_block must produce a multiple of the interpolation");
        for (auto& w : in) w.n_consumed = produced < 0 ? 0 : (produced / (int)_interp) * (int)_decim;
        return ret;
    }

private:
    unsigned _interp, _decim;
};

} // namespace gr
