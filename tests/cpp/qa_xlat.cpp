// rotator_cc and freq_xlating_fir_filter_ccf through the runtime.
//   XlatCpu.*  the CPU blocks (they define the semantics) on scheduler_mt with small buffers, so
//              the stream passes through many work() calls, against an in-test double reference
//              built on the 64-bit phase: turns(n) = ((n inc) mod 2^64 >> 11) / 2^53.
//   XlatHip.*  the GPU blocks in a scheduler_hip domain fed from / drained into a scheduler_mt
//              domain over H2D / D2H edges with 64 KiB rings, against the CPU blocks' output
//              (1e-5 norm-wise), restart, a time shard (set_first_index + set_initial_history) and
//              scheduler_hip's per-block kernel timing.
#include "qa.hpp"

#include <cmath>
#include <complex>
#include <gnuradio/blocklib/blocks/freq_xlating_fir_filter_ccf.hpp>
#include <gnuradio/blocklib/blocks/rotator_cc.hpp>
#include <gnuradio/blocklib/blocks/vector_sink.hpp>
#include <gnuradio/blocklib/blocks/vector_source.hpp>
#include <gnuradio/blocklib/hip/freq_xlating_fir_filter_ccf.hpp>
#include <gnuradio/blocklib/hip/rotator_cc.hpp>
#include <gnuradio/domain_adapter_direct.hpp>
#include <gnuradio/flowgraph.hpp>
#include <gnuradio/hip_buffer.hpp>
#include <gnuradio/schedulers/hip/scheduler_hip.hpp>
#include <gnuradio/schedulers/mt/scheduler_mt.hpp>

#include "nsh_hip.h"

using namespace gr;

#include "qa_ref.hpp"

namespace {

uint64_t inc_of(double turns)
{
    uint64_t inc = 0;
    EXPECT_EQ(nsh_phase_inc(turns, &inc), 0);
    return inc;
}
std::complex<double> phasor_ref(uint64_t n, uint64_t inc)
{
    const uint64_t p = n * inc; // mod 2^64
    const double turns = std::ldexp((double)(p >> 11), -53);
    return std::polar(1.0, 2.0 * M_PI * turns);
}
std::vector<gr_complex> rotate_ref(const std::vector<gr_complex>& x, uint64_t inc, uint64_t first)
{
    std::vector<gr_complex> y(x.size());
    for (size_t i = 0; i < x.size(); ++i) y[i] = gr_complex(std::complex<double>(x[i]) * phasor_ref(first + i, inc));
    return y;
}
// zero initial history
std::vector<gr_complex> xlat_ref(const std::vector<gr_complex>& x, const std::vector<float>& h, int D, uint64_t inc,
                                 uint64_t first)
{
    std::vector<std::complex<double>> r(x.size());
    for (size_t i = 0; i < x.size(); ++i) r[i] = std::complex<double>(x[i]) * phasor_ref(first + i, inc);
    std::vector<gr_complex> y(x.size() / D);
    for (size_t m = 0; m < y.size(); ++m) {
        std::complex<double> acc = 0;
        for (size_t k = 0; k < h.size(); ++k) {
            const long g = (long)(m * D) - (long)k;
            if (g >= 0) acc += (double)h[k] * r[g];
        }
        y[m] = gr_complex(acc);
    }
    return y;
}

// vector_source -> blk -> vector_sink on one scheduler_mt with small buffers; runs twice
std::vector<gr_complex> run_cpu(const block_sptr& blk, const std::vector<gr_complex>& x, bool check_rerun = true)
{
    auto src = blocks::vector_source_c::make(x);
    auto snk = blocks::vector_sink_c::make(1, x.size());
    auto fg = flowgraph::make();
    fg->connect(src, 0, blk, 0);
    fg->connect(blk, 0, snk, 0);
    fg->set_scheduler(schedulers::scheduler_mt::make("mt", 8192));
    fg->validate();
    fg->run();
    const auto y = snk->data();
    if (check_rerun) {
        fg->run(); // phase and history re-armed by start()
        EXPECT_TRUE(snk->data() == y);
    }
    return y;
}

struct hip_run {
    flowgraph_sptr fg;
    blocks::vector_sink_c::sptr snk;
    std::shared_ptr<schedulers::scheduler_hip> gpu;
};
// vector_source -[H2D]-> blk -[D2H]-> vector_sink: a scheduler_mt domain and a scheduler_hip domain, 64 KiB rings
hip_run make_hip(const block_sptr& blk, const std::vector<gr_complex>& x)
{
    hip_run r;
    auto src = blocks::vector_source_c::make(x);
    r.snk = blocks::vector_sink_c::make(1, x.size());
    r.fg = flowgraph::make();
    r.fg->connect(src, 0, blk, 0)->set_custom_buffer(HIP_BUFFER_ARGS_H2D);
    r.fg->connect(blk, 0, r.snk, 0)->set_custom_buffer(HIP_BUFFER_ARGS_D2H);
    auto cpu = schedulers::scheduler_mt::make("cpu", 1u << 16);
    r.gpu = schedulers::scheduler_hip::make("gpu", 0, 1u << 16);
    r.fg->add_scheduler(cpu);
    r.fg->add_scheduler(r.gpu);
    auto da = domain_adapter_direct_conf::make(buffer_preference_t::DOWNSTREAM);
    domain_conf_vec dc{ domain_conf(cpu, { src, r.snk }, da), domain_conf(r.gpu, { blk }, da) };
    r.fg->partition(dc);
    return r;
}

} // namespace

// ---- CPU blocks --------------------------------------------------------------------------------
TEST(XlatCpu, RotatorMatchesReference)
{
    const size_t n = 40000;
    const auto x = synth(n, 777);
    for (double f : { 0.1, 1e-9 })
        for (uint64_t first : { (uint64_t)0, (uint64_t)1 << 40 }) {
            auto rot = blocks::rotator_cc::make(2.0 * M_PI * f);
            rot->set_first_index(first);
            // the block's increment is that of its own frequency in turns, rad / 2 pi
            EXPECT_EQ(rot->phase_inc(), inc_of(2.0 * M_PI * f / (2.0 * M_PI)));
            const auto y = run_cpu(rot, x);
            EXPECT_TRUE(close_normwise(y, rotate_ref(x, rot->phase_inc(), first)));
            // and within the drift of rad / 2 pi against the exact frequency: 2^-52 f first turns
            if (first == 0) EXPECT_TRUE(close_normwise(y, rotate_ref(x, inc_of(f), 0)));
        }
}

static void xlat_cpu_case(int D, int L, double f, uint64_t first)
{
    const size_t n = (size_t)D * (D == 64 ? 600 : 9000) + 3; // the 3 odd inputs are never consumed
    const auto x = synth(n, 4242);
    const auto h = lowpass(L, 0.4 / D);
    auto blk = blocks::freq_xlating_fir_filter_ccf::make(D, h, f * 48000.0, 48000.0);
    blk->set_first_index(first);
    const auto y = run_cpu(blk, x);
    EXPECT_EQ(y.size(), n / D);
    EXPECT_EQ(blk->phase_inc(), inc_of(-(f * 48000.0 / 48000.0)));
    EXPECT_TRUE(close_normwise(y, xlat_ref(x, h, D, blk->phase_inc(), first)));
}
TEST(XlatCpu, XlatingFirD1L127) { xlat_cpu_case(1, 127, 0.1, 0); }
TEST(XlatCpu, XlatingFirD5L33) { xlat_cpu_case(5, 33, -0.37, ((uint64_t)1 << 40) + 7); }
TEST(XlatCpu, XlatingFirD64L200) { xlat_cpu_case(64, 200, 0.25, 0); }

// a tone at +center_freq lands at DC: the output is the filter's DC gain (1) times the tone's amplitude
TEST(XlatCpu, ToneAtCenterFreqLandsAtDc)
{
    const size_t n = 20000;
    const double f = 0.2;
    std::vector<gr_complex> x(n);
    const uint64_t inc = inc_of(f);
    for (size_t i = 0; i < n; ++i) x[i] = gr_complex(0.5 * phasor_ref(i, inc));
    const auto h = lowpass(65, 0.05);
    const auto y = run_cpu(blocks::freq_xlating_fir_filter_ccf::make(4, h, f, 1.0), x, false);
    ASSERT_TRUE(y.size() == n / 4);
    double worst = 0;
    for (size_t m = 32; m < y.size(); ++m) worst = std::max(worst, (double)std::abs(y[m] - gr_complex(0.5f, 0.f)));
    EXPECT_TRUE(worst < 1e-5);
}

// ---- GPU blocks --------------------------------------------------------------------------------
static void xlat_hip_case(int D, int L, double f)
{
    const size_t n = 300000;
    const auto x = synth(n, 99);
    const auto h = lowpass(L, 0.4 / D);
    const auto ref = run_cpu(blocks::freq_xlating_fir_filter_ccf::make(D, h, f, 1.0), x, false);
    auto blk = hip::freq_xlating_fir_filter_ccf::make(D, h, f, 1.0);
    auto r = make_hip(blk, x);
    r.fg->run();
    const auto y = r.snk->data();
    EXPECT_EQ(y.size(), n / D);
    EXPECT_TRUE(close_normwise(y, ref));
    EXPECT_EQ(blk->phase_inc(), inc_of(-f));
    std::printf("  D=%d L=%d: %s, %llu launches\n", D, L, blk->kernel().c_str(), (unsigned long long)blk->launches());
    EXPECT_TRUE(blk->launches() > 1);
    r.fg->run(); // phase and history re-armed by start()
    EXPECT_TRUE(r.snk->data() == y || close_normwise(r.snk->data(), ref));
}
TEST(XlatHip, FirD10L200MatchesCpuAndReruns) { xlat_hip_case(10, 200, 0.123); }
TEST(XlatHip, FirD16L127MatchesCpuAndReruns) { xlat_hip_case(16, 127, -0.3); }

TEST(XlatHip, RotatorMatchesCpuAndReruns)
{
    const size_t n = 300000;
    const auto x = synth(n, 5);
    const uint64_t first = ((uint64_t)1 << 40) + 7;
    auto cpu = blocks::rotator_cc::make(2.0 * M_PI * 0.123);
    cpu->set_first_index(first);
    const auto ref = run_cpu(cpu, x, false);
    auto blk = hip::rotator_cc::make(2.0 * M_PI * 0.123);
    blk->set_first_index(first);
    EXPECT_EQ(blk->phase_inc(), cpu->phase_inc());
    auto r = make_hip(blk, x);
    r.fg->run();
    const auto y = r.snk->data();
    EXPECT_TRUE(close_normwise(y, ref));
    EXPECT_TRUE(blk->launches() > 1);
    r.fg->run();
    EXPECT_TRUE(r.snk->data() == y || close_normwise(r.snk->data(), ref));
}

// a time shard: the stream from input n0 on, with the L-1 raw samples before it as initial history
// and first_index = n0, gives the tail of the whole stream's output
TEST(XlatHip, TimeShardReproducesTail)
{
    const int D = 10, L = 200;
    const size_t n = 300000, n0 = (size_t)D * 12345;
    const auto x = synth(n, 31);
    const auto h = lowpass(L, 0.04);
    const uint64_t base = ((uint64_t)1 << 40) + 7; // the whole stream starts here
    auto whole = hip::freq_xlating_fir_filter_ccf::make(D, h, 0.123, 1.0);
    whole->set_first_index(base);
    auto rw = make_hip(whole, x);
    rw.fg->run();
    const auto yw = rw.snk->data();
    ASSERT_TRUE(yw.size() == n / D);

    auto shard = hip::freq_xlating_fir_filter_ccf::make(D, h, 0.123, 1.0);
    shard->set_first_index(base + n0);
    shard->set_initial_history(std::vector<gr_complex>(x.begin() + (n0 - (L - 1)), x.begin() + n0));
    auto rs = make_hip(shard, std::vector<gr_complex>(x.begin() + n0, x.end()));
    rs.fg->run();
    const auto ys = rs.snk->data();
    EXPECT_TRUE(close_normwise(ys, std::vector<gr_complex>(yw.begin() + n0 / D, yw.end())));
    // without the first index the shard is a different signal
    auto wrong = hip::freq_xlating_fir_filter_ccf::make(D, h, 0.123, 1.0);
    wrong->set_initial_history(std::vector<gr_complex>(x.begin() + (n0 - (L - 1)), x.begin() + n0));
    auto rx = make_hip(wrong, std::vector<gr_complex>(x.begin() + n0, x.end()));
    rx.fg->run();
    double d = 0;
    const auto yx = rx.snk->data();
    for (size_t i = 0; i < std::min(ys.size(), yx.size()); ++i) d = std::max(d, (double)std::abs(ys[i] - yx[i]));
    EXPECT_TRUE(d > 1e-3);
}

// scheduler_hip's per-block kernel timing needs nothing from the blocks: one nsh::launch per work()
TEST(XlatHip, KernelTimingOneLaunchPerWork)
{
    const size_t n = 300000;
    const auto x = synth(n, 8);
    for (int which = 0; which < 2; ++which) {
        block_sptr blk;
        std::function<uint64_t()> launches;
        uint64_t items = 0;
        if (which == 0) {
            auto b = hip::freq_xlating_fir_filter_ccf::make(16, lowpass(127, 0.02), -0.3, 1.0);
            launches = [b] { return b->launches(); };
            items = n / 16;
            blk = b;
        } else {
            auto b = hip::rotator_cc::make(0.7);
            launches = [b] { return b->launches(); };
            items = n;
            blk = b;
        }
        auto r = make_hip(blk, x);
        r.gpu->set_kernel_timing(true);
        r.fg->run();
        const auto st = r.gpu->kernel_stats();
        size_t found = 0;
        for (auto& k : st) {
            if (k.block.find(which == 0 ? "freq_xlating_fir_filter_ccf" : "rotator_cc") == std::string::npos) continue;
            ++found;
            EXPECT_EQ(k.launches, launches());
            EXPECT_EQ(k.items, items);
            EXPECT_TRUE(k.kernel_ms > 0);
        }
        EXPECT_EQ(found, (size_t)1);
    }
}
