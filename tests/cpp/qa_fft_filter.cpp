// fft_filter_ccc / fft_filter_ccf through the runtime.
//   FftFilterCpu.*  the CPU block (it defines the semantics) on scheduler_mt with small buffers, so the
//                   stream passes through many work() calls, against an in-test double convolution, and
//                   what the constructors of both blocks refuse.
//   FftFilterHip.*  the GPU blocks in a scheduler_hip domain fed from / drained into a scheduler_mt
//                   domain over H2D / D2H edges with 64 KiB rings (work() calls that are no multiples of
//                   the frames' valid length), against the CPU block's output: complex and real taps at
//                   two frame sizes, a restart from zero history, a time shard, and the kernel timing of
//                   the scheduler and of the block.
// Tolerance: per output |y - r| <= 1e-5 |r| + 1e-6 max|x| sum|h| with the maximum over the whole
// stream (the header's bound takes it over the output's frame; tests/test_gpu_fft_filter.py checks
// that one, frame by frame).
#include "qa.hpp"

#include <cmath>
#include <complex>
#include <stdexcept>
#include <gnuradio/blocklib/blocks/fft_filter.hpp>
#include <gnuradio/blocklib/blocks/vector_sink.hpp>
#include <gnuradio/blocklib/blocks/vector_source.hpp>
#include <gnuradio/blocklib/hip/fft_filter.hpp>
#include <gnuradio/domain_adapter_direct.hpp>
#include <gnuradio/flowgraph.hpp>
#include <gnuradio/hip_buffer.hpp>
#include <gnuradio/schedulers/hip/scheduler_hip.hpp>
#include <gnuradio/schedulers/mt/scheduler_mt.hpp>

#include "nsh_hip.h"

using namespace gr;

#include "qa_ref.hpp"

namespace {

// zero initial history, accumulated in double
std::vector<gr_complex> conv_ref(const std::vector<gr_complex>& x, const std::vector<gr_complex>& h)
{
    std::vector<gr_complex> y(x.size());
    for (size_t i = 0; i < x.size(); ++i) {
        std::complex<double> acc = 0;
        for (size_t k = 0; k < h.size() && k <= i; ++k) acc += std::complex<double>(h[k]) * std::complex<double>(x[i - k]);
        y[i] = gr_complex(acc);
    }
    return y;
}

bool within_bound(const std::vector<gr_complex>& y, const std::vector<gr_complex>& r, const std::vector<gr_complex>& x,
                  const std::vector<gr_complex>& h)
{
    if (y.size() != r.size()) {
        std::fprintf(stderr, "  size %zu != %zu\n", y.size(), r.size());
        return false;
    }
    double xmax = 0, hsum = 0, worst = 0;
    for (auto& v : x) xmax = std::max(xmax, (double)std::abs(v));
    for (auto& v : h) hsum += std::abs(std::complex<double>(v));
    for (size_t i = 0; i < y.size(); ++i) {
        const double b = 1e-5 * std::abs(r[i]) + 1e-6 * xmax * hsum;
        worst = std::max(worst, (double)std::abs(y[i] - r[i]) / b);
    }
    if (!(worst <= 1.0)) std::fprintf(stderr, "  worst err / bound %g\n", worst);
    return worst <= 1.0;
}

// taps without symmetry: the stream generator at another seed, scaled
std::vector<gr_complex> complex_taps(size_t L)
{
    auto h = synth(L, 0, 0x7461707300ull);
    for (auto& v : h) v *= 1.0f / 16.0f;
    return h;
}
std::vector<gr_complex> as_complex(const std::vector<float>& h) { return std::vector<gr_complex>(h.begin(), h.end()); }

// vector_source -> blk -> vector_sink on one scheduler_mt with small buffers; runs twice
std::vector<gr_complex> run_cpu(const block_sptr& blk, const std::vector<gr_complex>& x, bool check_rerun = true)
{
    auto src = blocks::vector_source_c::make(x, false, 1u);
    auto snk = blocks::vector_sink_c::make(1, x.size());
    auto fg = flowgraph::make();
    fg->connect(src, 0, blk, 0);
    fg->connect(blk, 0, snk, 0);
    fg->set_scheduler(schedulers::scheduler_mt::make("mt", 8192));
    fg->validate();
    fg->run();
    const auto y = snk->data();
    if (check_rerun) {
        fg->run(); // history re-armed by start()
        EXPECT_TRUE(snk->data() == y);
    }
    return y;
}

struct hip_run {
    flowgraph_sptr fg;
    blocks::vector_sink_c::sptr snk;
    std::shared_ptr<schedulers::scheduler_hip> gpu;
};
// vector_source -[H2D]-> blk -[D2H]-> vector_sink: a scheduler_mt domain and a scheduler_hip domain,
// 64 KiB rings
hip_run make_hip(const block_sptr& blk, const std::vector<gr_complex>& x)
{
    hip_run r;
    auto src = blocks::vector_source_c::make(x, false, 1u);
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

template <class F>
bool refused(F make)
{
    try {
        make();
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}

} // namespace

// ---- CPU block ---------------------------------------------------------------------------------
static void cpu_case(size_t L, size_t n)
{
    const auto x = synth(n, 777);
    const auto h = complex_taps(L);
    const auto y = run_cpu(blocks::fft_filter_ccc::make(h), x);
    EXPECT_EQ(y.size(), n);
    EXPECT_TRUE(within_bound(y, conv_ref(x, h), x, h));
}
TEST(FftFilterCpu, L1) { cpu_case(1, 20000); }
TEST(FftFilterCpu, L127) { cpu_case(127, 30000); }
TEST(FftFilterCpu, L1000) { cpu_case(1000, 20000); }

TEST(FftFilterCpu, RefusesBadArguments)
{
    const float nan = std::nanf(""), inf = INFINITY;
    EXPECT_TRUE(refused([] { blocks::fft_filter_ccc::make({}); }));
    EXPECT_TRUE(refused([] { blocks::fft_filter_ccc::make(complex_taps(4097)); }));
    EXPECT_TRUE(refused([&] { blocks::fft_filter_ccc::make({ gr_complex(1, 0), gr_complex(0, nan) }); }));
    EXPECT_FALSE(refused([] { blocks::fft_filter_ccc::make(complex_taps(4096)); }));
    // what the plan refuses, refused by the GPU blocks' constructors (no device needed)
    EXPECT_TRUE(refused([] { hip::fft_filter_ccc::make({}); }));
    EXPECT_TRUE(refused([] { hip::fft_filter_ccc::make(complex_taps(4097)); }));
    EXPECT_TRUE(refused([&] { hip::fft_filter_ccc::make({ gr_complex(inf, 0) }); }));
    EXPECT_TRUE(refused([] { hip::fft_filter_ccc::make(complex_taps(3), 512); }));
    EXPECT_TRUE(refused([] { hip::fft_filter_ccc::make(complex_taps(3), 3000); }));
    EXPECT_TRUE(refused([] { hip::fft_filter_ccc::make(complex_taps(513), 1024); }));
    EXPECT_TRUE(refused([] { hip::fft_filter_ccf::make({}); }));
    EXPECT_TRUE(refused([&] { hip::fft_filter_ccf::make({ 1.f, nan }); }));
    EXPECT_TRUE(refused([] { hip::fft_filter_ccf::make(lowpass(2049, 0.1), 4096); }));
    EXPECT_FALSE(refused([] { hip::fft_filter_ccc::make(complex_taps(512), 1024); }));
    EXPECT_FALSE(refused([] { hip::fft_filter_ccf::make(lowpass(4096, 0.1)); }));
}

// ---- GPU blocks --------------------------------------------------------------------------------
static void hip_case(const std::shared_ptr<hip::fft_filter_ccc>& blk, const std::vector<gr_complex>& h, size_t want_size)
{
    const size_t n = 100000;
    const auto x = synth(n, 4242);
    const auto ref = run_cpu(blocks::fft_filter_ccc::make(h), x, false);
    auto r = make_hip(blk, x);
    r.fg->run();
    const auto y = r.snk->data();
    EXPECT_EQ(y.size(), n);
    EXPECT_TRUE(within_bound(y, ref, x, h));
    EXPECT_EQ(blk->fft_size(), want_size);
    std::printf("  L=%zu: %s, %llu launches\n", h.size(), blk->kernel().c_str(), (unsigned long long)blk->launches());
    EXPECT_TRUE(blk->launches() > 1);
    // a restart starts from zero history: the reference's first ntaps-1 outputs again, which the last
    // run's tail as history would change
    r.fg->run();
    const auto y2 = r.snk->data();
    EXPECT_TRUE(within_bound(y2, ref, x, h));
}
TEST(FftFilterHip, ComplexTapsDefaultSize)
{
    const auto h = complex_taps(127);
    hip_case(hip::fft_filter_ccc::make(h), h, 1024);
}
TEST(FftFilterHip, ComplexTapsSize4096)
{
    const auto h = complex_taps(1500);
    hip_case(hip::fft_filter_ccc::make(h, 4096), h, 4096);
}
TEST(FftFilterHip, RealTapsDefaultSize)
{
    const auto h = lowpass(255, 0.1);
    hip_case(hip::fft_filter_ccf::make(h), as_complex(h), 1024);
}
TEST(FftFilterHip, RealTapsSize4096)
{
    const auto h = lowpass(1024, 0.05);
    hip_case(hip::fft_filter_ccf::make(h, 4096), as_complex(h), 4096);
}

// a time shard: the stream from sample n0 on, with the ntaps-1 raw samples before it as initial
// history, gives the tail of the whole stream's output
TEST(FftFilterHip, TimeShardReproducesTail)
{
    const size_t n = 60000, n0 = 23457, L = 300;
    const auto x = synth(n, 31);
    const auto h = complex_taps(L);
    const auto ref = conv_ref(x, h);
    auto shard = hip::fft_filter_ccc::make(h);
    shard->set_initial_history(std::vector<gr_complex>(x.begin() + (n0 - (L - 1)), x.begin() + n0));
    const std::vector<gr_complex> xs(x.begin() + n0, x.end());
    auto rs = make_hip(shard, xs);
    rs.fg->run();
    EXPECT_TRUE(within_bound(rs.snk->data(), std::vector<gr_complex>(ref.begin() + n0, ref.end()), x, h));
}

// scheduler_hip's per-block kernel timing needs nothing from the block (one nsh::launch per work());
// the block's own timing arms a pair per launch
TEST(FftFilterHip, KernelTimingOneLaunchPerWork)
{
    const size_t n = 200000;
    const auto x = synth(n, 9);
    auto blk = hip::fft_filter_ccc::make(complex_taps(127));
    auto r = make_hip(blk, x);
    r.gpu->set_kernel_timing(true);
    r.fg->run();
    const auto st = r.gpu->kernel_stats();
    size_t found = 0;
    for (auto& k : st) {
        if (k.block.find("fft_filter_ccc") == std::string::npos) continue;
        ++found;
        EXPECT_EQ(k.launches, blk->launches());
        EXPECT_EQ(k.items, (uint64_t)n);
        EXPECT_TRUE(k.kernel_ms > 0);
    }
    EXPECT_EQ(found, (size_t)1);
    r.gpu->set_kernel_timing(false);
    blk->enable_timing(true);
    r.fg->run();
    EXPECT_EQ(blk->timed_samples(), (uint64_t)n);
    EXPECT_TRUE(blk->kernel_ms() > 0); // throws if an armed pair went unrecorded
}
