// freq_xlating_fft_filter_ccc / _ccf through the runtime.
//   FftXlatCpu.*  the CPU block (it defines the semantics) on scheduler_mt with small buffers, so the
//                 stream passes through many work() calls, against an in-test double sum of the
//                 definition, and what the constructors of both blocks refuse.
//   FftXlatHip.*  the GPU blocks in a scheduler_hip domain fed from / drained into a scheduler_mt
//                 domain over H2D / D2H edges with 64 KiB rings (work() calls that are no multiples of
//                 the frames' Vd outputs), against the CPU block's output: complex and real taps at two
//                 (N, D), a restart from zero history, and a time shard with set_first_index.
// Tolerance: per output |y - r| <= 1e-5 |r| + 1e-6 max|x| sum|h| with the maximum over the whole
// stream (the header's bound takes it over the output's frame; tests/test_gpu_fft_xlat.py checks
// that one, frame by frame).
#include "qa.hpp"

#include <cmath>
#include <complex>
#include <stdexcept>
#include <gnuradio/blocklib/blocks/freq_xlating_fft_filter_ccc.hpp>
#include <gnuradio/blocklib/blocks/vector_sink.hpp>
#include <gnuradio/blocklib/blocks/vector_source.hpp>
#include <gnuradio/blocklib/hip/freq_xlating_fft_filter_ccc.hpp>
#include <gnuradio/domain_adapter_direct.hpp>
#include <gnuradio/flowgraph.hpp>
#include <gnuradio/hip_buffer.hpp>
#include <gnuradio/schedulers/hip/scheduler_hip.hpp>
#include <gnuradio/schedulers/mt/scheduler_mt.hpp>

#include "nsh_hip.h"

using namespace gr;

#include "qa_ref.hpp"

namespace {

// y[m] = sum_k h[k] x[mD-k] exp(j 2 pi phase(first + mD - k)), zero initial history, in double
std::vector<gr_complex> xlat_ref(const std::vector<gr_complex>& x, const std::vector<gr_complex>& h, int D, double freq_norm,
                                 uint64_t first = 0)
{
    uint64_t inc = 0;
    EXPECT_EQ(nsh_phase_inc(-freq_norm, &inc), 0);
    std::vector<std::complex<double>> rot(x.size());
    for (size_t i = 0; i < x.size(); ++i) {
        const double th = 2.0 * M_PI * std::ldexp((double)(int64_t)((first + (uint64_t)i) * inc), -64);
        rot[i] = std::complex<double>(x[i]) * std::complex<double>(std::cos(th), std::sin(th));
    }
    std::vector<gr_complex> y(x.size() / D);
    for (size_t m = 0; m < y.size(); ++m) {
        std::complex<double> acc = 0;
        for (size_t k = 0; k < h.size() && k <= m * D; ++k) acc += std::complex<double>(h[k]) * rot[m * D - k];
        y[m] = gr_complex(acc);
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
std::vector<gr_complex> run_cpu(const block_sptr& blk, const std::vector<gr_complex>& x, size_t n_out, bool check_rerun = true)
{
    auto src = blocks::vector_source_c::make(x, false, 1u);
    auto snk = blocks::vector_sink_c::make(1, n_out);
    auto fg = flowgraph::make();
    fg->connect(src, 0, blk, 0);
    fg->connect(blk, 0, snk, 0);
    fg->set_scheduler(schedulers::scheduler_mt::make("mt", 8192));
    fg->validate();
    fg->run();
    const auto y = snk->data();
    if (check_rerun) {
        fg->run(); // history and sample counter re-armed by start()
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
hip_run make_hip(const block_sptr& blk, const std::vector<gr_complex>& x, size_t n_out)
{
    hip_run r;
    auto src = blocks::vector_source_c::make(x, false, 1u);
    r.snk = blocks::vector_sink_c::make(1, n_out);
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
static void cpu_case(size_t L, int D, double f, size_t n)
{
    const auto x = synth(n, 777);
    const auto h = complex_taps(L);
    const auto y = run_cpu(blocks::freq_xlating_fft_filter_ccc::make(D, h, f, 1.0), x, n / D);
    EXPECT_EQ(y.size(), n / D);
    EXPECT_TRUE(within_bound(y, xlat_ref(x, h, D, f), x, h));
}
TEST(FftXlatCpu, L1D1) { cpu_case(1, 1, 0.1, 20000); }
TEST(FftXlatCpu, L127D8) { cpu_case(127, 8, -0.21, 32000); }
TEST(FftXlatCpu, L1000D64) { cpu_case(1000, 64, 0.37, 64000); }

TEST(FftXlatCpu, RefusesBadArguments)
{
    const float nan = std::nanf(""), inf = INFINITY;
    const auto h3 = complex_taps(3);
    EXPECT_TRUE(refused([] { blocks::freq_xlating_fft_filter_ccc::make(2, {}, 0.1, 1.0); }));
    EXPECT_TRUE(refused([] { blocks::freq_xlating_fft_filter_ccc::make(2, complex_taps(4097), 0.1, 1.0); }));
    EXPECT_TRUE(refused([&] { blocks::freq_xlating_fft_filter_ccc::make(2, { gr_complex(1, 0), gr_complex(0, nan) }, 0.1, 1.0); }));
    EXPECT_TRUE(refused([&] { blocks::freq_xlating_fft_filter_ccc::make(3, h3, 0.1, 1.0); }));
    EXPECT_TRUE(refused([&] { blocks::freq_xlating_fft_filter_ccc::make(0, h3, 0.1, 1.0); }));
    EXPECT_TRUE(refused([&] { blocks::freq_xlating_fft_filter_ccc::make(128, h3, 0.1, 1.0); }));
    EXPECT_TRUE(refused([&] { blocks::freq_xlating_fft_filter_ccc::make(2, h3, 0.1, 0.0); }));
    EXPECT_TRUE(refused([&] { blocks::freq_xlating_fft_filter_ccc::make(2, h3, (double)inf, 1.0); }));
    EXPECT_FALSE(refused([] { blocks::freq_xlating_fft_filter_ccc::make(64, complex_taps(4096), -0.3, 2.0); }));
    // what the plan refuses, refused by the GPU blocks' constructors (no device needed)
    EXPECT_TRUE(refused([] { hip::freq_xlating_fft_filter_ccc::make(2, {}, 0.1, 1.0); }));
    EXPECT_TRUE(refused([] { hip::freq_xlating_fft_filter_ccc::make(2, complex_taps(4097), 0.1, 1.0); }));
    EXPECT_TRUE(refused([&] { hip::freq_xlating_fft_filter_ccc::make(2, { gr_complex(inf, 0) }, 0.1, 1.0); }));
    EXPECT_TRUE(refused([&] { hip::freq_xlating_fft_filter_ccc::make(3, h3, 0.1, 1.0); }));
    EXPECT_TRUE(refused([&] { hip::freq_xlating_fft_filter_ccc::make(0, h3, 0.1, 1.0); }));
    EXPECT_TRUE(refused([&] { hip::freq_xlating_fft_filter_ccc::make(128, h3, 0.1, 1.0); }));
    EXPECT_TRUE(refused([&] { hip::freq_xlating_fft_filter_ccc::make(2, h3, 0.1, -1.0); }));
    EXPECT_TRUE(refused([&] { hip::freq_xlating_fft_filter_ccc::make(2, h3, (double)nan, 1.0); }));
    EXPECT_TRUE(refused([&] { hip::freq_xlating_fft_filter_ccc::make(2, h3, 0.1, 1.0, 512); }));
    EXPECT_TRUE(refused([&] { hip::freq_xlating_fft_filter_ccc::make(2, h3, 0.1, 1.0, 3000); }));
    EXPECT_TRUE(refused([] { hip::freq_xlating_fft_filter_ccc::make(2, complex_taps(513), 0.1, 1.0, 1024); }));
    EXPECT_TRUE(refused([] { hip::freq_xlating_fft_filter_ccf::make(2, {}, 0.1, 1.0); }));
    EXPECT_TRUE(refused([&] { hip::freq_xlating_fft_filter_ccf::make(2, { 1.f, nan }, 0.1, 1.0); }));
    EXPECT_TRUE(refused([] { hip::freq_xlating_fft_filter_ccf::make(2, lowpass(2049, 0.1), 0.1, 1.0, 4096); }));
    EXPECT_FALSE(refused([] { hip::freq_xlating_fft_filter_ccc::make(64, complex_taps(512), 0.1, 1.0, 1024); }));
    EXPECT_FALSE(refused([] { hip::freq_xlating_fft_filter_ccf::make(1, lowpass(4096, 0.1), 0.0, 1.0); }));
}

// ---- GPU blocks --------------------------------------------------------------------------------
static void hip_case(const std::shared_ptr<hip::freq_xlating_fft_filter_ccc>& blk, const std::vector<gr_complex>& h, int D,
                     double f, size_t want_size, const std::string& want_kernel)
{
    const size_t n = 1u << 17, n_out = n / D;
    const auto x = synth(n, 4242);
    const auto ref = run_cpu(blocks::freq_xlating_fft_filter_ccc::make(D, h, f, 1.0), x, n_out, false);
    auto r = make_hip(blk, x, n_out);
    r.fg->run();
    const auto y = r.snk->data();
    EXPECT_EQ(y.size(), n_out);
    EXPECT_TRUE(within_bound(y, ref, x, h));
    EXPECT_EQ(blk->fft_size(), want_size);
    EXPECT_TRUE(blk->kernel() == want_kernel);
    uint64_t inc = 0;
    EXPECT_EQ(nsh_phase_inc(-f, &inc), 0);
    EXPECT_EQ(blk->phase_inc(), inc);
    std::printf("  L=%zu D=%d: %s, %llu launches\n", h.size(), D, blk->kernel().c_str(), (unsigned long long)blk->launches());
    EXPECT_TRUE(blk->launches() > 1);
    // a restart starts from zero history and the first index again
    r.fg->run();
    EXPECT_TRUE(within_bound(r.snk->data(), ref, x, h));
}
TEST(FftXlatHip, ComplexTaps1024D8)
{
    const auto h = complex_taps(127);
    hip_case(hip::freq_xlating_fft_filter_ccc::make(8, h, 0.123, 1.0), h, 8, 0.123, 1024, "k_fft_xlat<1024, 8>");
}
TEST(FftXlatHip, ComplexTaps4096D2)
{
    const auto h = complex_taps(1500);
    hip_case(hip::freq_xlating_fft_filter_ccc::make(2, h, -0.31, 1.0, 4096), h, 2, -0.31, 4096, "k_fft_xlat<4096, 2>");
}
TEST(FftXlatHip, RealTaps1024D8)
{
    const auto h = lowpass(255, 0.05);
    hip_case(hip::freq_xlating_fft_filter_ccf::make(8, h, 0.123, 1.0), as_complex(h), 8, 0.123, 1024, "k_fft_xlat<1024, 8>");
}
TEST(FftXlatHip, RealTaps4096D2)
{
    const auto h = lowpass(1024, 0.2);
    hip_case(hip::freq_xlating_fft_filter_ccf::make(2, h, -0.31, 1.0, 4096), as_complex(h), 2, -0.31, 4096, "k_fft_xlat<4096, 2>");
}

// a time shard: the stream from sample n0 on (a multiple of D), with the ntaps-1 raw samples before it
// as initial history and n0 as first index, gives the tail of the whole stream's output
TEST(FftXlatHip, TimeShardReproducesTail)
{
    const int D = 4;
    const size_t n = 1u << 16, n0 = 23456, L = 300;
    const double f = 0.2371;
    const auto x = synth(n, 31);
    const auto h = complex_taps(L);
    const auto ref = xlat_ref(x, h, D, f);
    auto shard = hip::freq_xlating_fft_filter_ccc::make(D, h, f, 1.0);
    shard->set_initial_history(std::vector<gr_complex>(x.begin() + (n0 - (L - 1)), x.begin() + n0));
    shard->set_first_index(n0);
    const std::vector<gr_complex> xs(x.begin() + n0, x.end());
    auto rs = make_hip(shard, xs, (n - n0) / D);
    rs.fg->run();
    EXPECT_TRUE(within_bound(rs.snk->data(), std::vector<gr_complex>(ref.begin() + n0 / D, ref.end()), x, h));
}
