// fft_vcc through the runtime.
//   FftCpu.*  the CPU block (it defines the semantics) on scheduler_mt with small buffers, against an
//             in-test O(N^2) double DFT written from the conventions (window on the input as it
//             arrives, forward shift on the output, inverse shift on the input) at N = 16 and 64, its
//             own round trip at 4096, and the refusals of both blocks.
//   FftHip.*  the GPU block in a scheduler_hip domain fed from / drained into a scheduler_mt domain
//             over H2D / D2H edges with 64 KiB rings, against the CPU block (1e-5 norm-wise); the
//             channelizer fusion takes fwd -> multiply_const_vcc -> inv only at 1024 points without
//             window and shift; scheduler_hip's kernel timing names the FFT launch.
#include "qa.hpp"

#include <cmath>
#include <complex>
#include <stdexcept>
#include <gnuradio/blocklib/blocks/fft.hpp>
#include <gnuradio/blocklib/blocks/vector_sink.hpp>
#include <gnuradio/blocklib/blocks/vector_source.hpp>
#include <gnuradio/blocklib/hip/fft.hpp>
#include <gnuradio/blocklib/hip/multiply_const.hpp>
#include <gnuradio/domain_adapter_direct.hpp>
#include <gnuradio/flowgraph.hpp>
#include <gnuradio/hip_buffer.hpp>
#include <gnuradio/schedulers/hip/scheduler_hip.hpp>
#include <gnuradio/schedulers/mt/scheduler_mt.hpp>

#include "nsh_hip.h"

using namespace gr;

#include "qa_ref.hpp"

namespace {

std::vector<float> hann(size_t N)
{
    std::vector<float> w(N);
    for (size_t n = 0; n < N; ++n) w[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)n / (double)N));
    return w;
}
// positive and negative entries, no symmetry
std::vector<float> ramp_window(size_t N)
{
    std::vector<float> w(N);
    for (size_t n = 0; n < N; ++n) w[n] = (float)(((double)((n * 37 + 11) % N) - 0.4 * (double)N) / (double)N);
    return w;
}

// the conventions, from the definition, in double
std::vector<gr_complex> dft_ref(const std::vector<gr_complex>& x, size_t N, bool forward, const std::vector<float>& w, bool shift)
{
    std::vector<gr_complex> y(x.size());
    std::vector<std::complex<double>> a(N);
    for (size_t f = 0; f + N <= x.size(); f += N) {
        for (size_t n = 0; n < N; ++n) {
            const size_t src = !forward && shift ? (n + N / 2) % N : n;
            const float wv = w.empty() ? 1.f : w[src];
            a[n] = { (double)(x[f + src].real() * wv), (double)(x[f + src].imag() * wv) };
        }
        for (size_t k = 0; k < N; ++k) {
            const size_t bin = forward && shift ? (k + N / 2) % N : k;
            std::complex<double> s = 0;
            for (size_t n = 0; n < N; ++n)
                s += a[n] * std::polar(1.0, (forward ? -2.0 : 2.0) * M_PI * (double)((bin * n) % N) / (double)N);
            y[f + k] = gr_complex(s);
        }
    }
    return y;
}

// vector_source(vlen N) -> blks -> vector_sink(vlen N) on one scheduler_mt with small buffers
std::vector<gr_complex> run_cpu(const std::vector<block_sptr>& blks, const std::vector<gr_complex>& x, size_t N)
{
    auto src = blocks::vector_source_c::make(x, false, (unsigned)N);
    auto snk = blocks::vector_sink_c::make(N, x.size() / N);
    auto fg = flowgraph::make();
    fg->connect(src, 0, blks.front(), 0);
    for (size_t i = 0; i + 1 < blks.size(); ++i) fg->connect(blks[i], 0, blks[i + 1], 0);
    fg->connect(blks.back(), 0, snk, 0);
    fg->set_scheduler(schedulers::scheduler_mt::make("mt", (unsigned)std::max<size_t>(8192, 4 * N * sizeof(gr_complex))));
    fg->validate();
    fg->run();
    return snk->data();
}

struct hip_run {
    flowgraph_sptr fg;
    blocks::vector_sink_c::sptr snk;
    std::shared_ptr<schedulers::scheduler_hip> gpu;
};
// vector_source(vlen N) -[H2D]-> blks, device edges between them -[D2H]-> vector_sink(vlen N):
// a scheduler_mt domain and a scheduler_hip domain, 64 KiB rings (8 items where those are larger)
hip_run make_hip(const std::vector<block_sptr>& blks, const std::vector<gr_complex>& x, size_t N)
{
    hip_run r;
    auto src = blocks::vector_source_c::make(x, false, (unsigned)N);
    r.snk = blocks::vector_sink_c::make(N, x.size() / N);
    r.fg = flowgraph::make();
    r.fg->connect(src, 0, blks.front(), 0)->set_custom_buffer(HIP_BUFFER_ARGS_H2D);
    for (size_t i = 0; i + 1 < blks.size(); ++i) r.fg->connect(blks[i], 0, blks[i + 1], 0)->set_custom_buffer(HIP_BUFFER_ARGS_D2D);
    r.fg->connect(blks.back(), 0, r.snk, 0)->set_custom_buffer(HIP_BUFFER_ARGS_D2H);
    const unsigned ring = (unsigned)std::max<size_t>(1u << 16, 8 * N * sizeof(gr_complex)); // at least 8 items
    auto cpu = schedulers::scheduler_mt::make("cpu", ring);
    r.gpu = schedulers::scheduler_hip::make("gpu", 0, ring);
    r.fg->add_scheduler(cpu);
    r.fg->add_scheduler(r.gpu);
    auto da = domain_adapter_direct_conf::make(buffer_preference_t::DOWNSTREAM);
    domain_conf_vec dc{ domain_conf(cpu, { src, r.snk }, da),
                        domain_conf(r.gpu, std::vector<node_sptr>(blks.begin(), blks.end()), da) };
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
static void cpu_case(size_t N, bool forward, bool window, bool shift)
{
    const auto x = synth(N * 37, 4243 + N);
    const auto w = window ? ramp_window(N) : std::vector<float>{};
    auto blk = blocks::fft_vcc::make(N, forward, w, shift);
    EXPECT_EQ(blk->fft_size(), N);
    EXPECT_TRUE(blk->forward() == forward && blk->shift() == shift && blk->window() == w);
    const auto y = run_cpu({ blk }, x, N);
    ASSERT_TRUE(y.size() == x.size());
    EXPECT_TRUE(close_normwise(y, dft_ref(x, N, forward, w, shift)));
}
TEST(FftCpu, N16AgainstDft)
{
    for (int v = 0; v < 8; ++v) cpu_case(16, v & 1, v & 2, v & 4);
}
TEST(FftCpu, N64AgainstDft)
{
    for (int v = 0; v < 8; ++v) cpu_case(64, v & 1, v & 2, v & 4);
}
// inverse(forward(x)) = N x at 4096, plain and with the two shifts (they cancel: the forward's output
// shift is undone by the inverse's input shift)
TEST(FftCpu, N4096RoundTrip)
{
    const size_t N = 4096;
    const auto x = synth(N * 5, 77);
    for (int shift = 0; shift < 2; ++shift) {
        const auto y = run_cpu({ blocks::fft_vcc::make(N, true, {}, shift), blocks::fft_vcc::make(N, false, {}, shift) }, x, N);
        ASSERT_TRUE(y.size() == x.size());
        std::vector<gr_complex> z(y.size());
        for (size_t i = 0; i < y.size(); ++i) z[i] = y[i] / (float)N;
        EXPECT_TRUE(close_normwise(z, x));
    }
}
TEST(FftCpu, RefusesBadArguments)
{
    for (size_t bad : { (size_t)0, (size_t)8, (size_t)24, (size_t)1000, (size_t)16384 }) {
        EXPECT_TRUE(refused([bad] { blocks::fft_vcc::make(bad); }));
        EXPECT_TRUE(refused([bad] { hip::fft_vcc::make(bad); }));
    }
    EXPECT_TRUE(refused([] { blocks::fft_vcc::make(64, true, std::vector<float>(63, 1.f)); }));
    EXPECT_TRUE(refused([] { blocks::fft_vcc::make(64, false, std::vector<float>(128, 1.f)); }));
    EXPECT_TRUE(refused([] { hip::fft_vcc::make(64, true, std::vector<float>(63, 1.f)); }));
    EXPECT_TRUE(refused([] { hip::fft_vcc::make(1024, false, std::vector<float>(1, 1.f), true); }));
    for (size_t ok : { (size_t)16, (size_t)1024, (size_t)8192 }) {
        EXPECT_FALSE(refused([ok] { blocks::fft_vcc::make(ok, true, std::vector<float>(ok, 1.f), true); }));
        EXPECT_FALSE(refused([ok] { hip::fft_vcc::make(ok, false, std::vector<float>(ok, 1.f), true); }));
    }
    auto h = hip::fft_vcc::make(2048, false, hann(2048), true);
    EXPECT_EQ(h->fft_size(), (size_t)2048);
    EXPECT_TRUE(!h->forward() && h->shift() && h->window() == hann(2048));
    auto d = hip::fft_vcc::make(); // the old call: 1024, forward, plain
    EXPECT_EQ(d->fft_size(), (size_t)1024);
    EXPECT_TRUE(d->forward() && !d->shift() && d->window().empty());
}

// ---- GPU block ---------------------------------------------------------------------------------
static void hip_case(size_t N, bool forward, const std::vector<float>& w, bool shift, size_t frames)
{
    const auto x = synth(N * frames, 98 + N);
    const auto ref = run_cpu({ blocks::fft_vcc::make(N, forward, w, shift) }, x, N);
    auto r = make_hip({ hip::fft_vcc::make(N, forward, w, shift) }, x, N);
    r.fg->run();
    const auto y = r.snk->data();
    ASSERT_TRUE(y.size() == x.size());
    EXPECT_TRUE(close_normwise(y, ref));
    r.fg->run(); // the plan survives a restart
    EXPECT_TRUE(r.snk->data() == y);
}
TEST(FftHip, N16MatchesCpu)
{
    hip_case(16, true, {}, false, 5001);
    hip_case(16, false, ramp_window(16), true, 777);
}
TEST(FftHip, N256MatchesCpu)
{
    hip_case(256, true, {}, false, 1001);
    hip_case(256, false, {}, true, 333);
}
TEST(FftHip, N1024HannShiftMatchesCpu)
{
    hip_case(1024, true, hann(1024), true, 301);
    hip_case(1024, false, hann(1024), true, 37);
}
TEST(FftHip, N4096MatchesCpu)
{
    hip_case(4096, true, {}, false, 67);
    hip_case(4096, false, hann(4096), false, 21);
}

// fwd -> multiply_const_vcc(k) -> inv on one scheduler_hip; returns the number of fused blocks
static size_t chain_case(size_t N, const std::vector<float>& w, bool shift)
{
    const size_t frames = 61;
    const auto x = synth(N * frames, 5 + N);
    std::vector<gr_complex> k(N);
    for (size_t b = 0; b < N; ++b) k[b] = gr_complex((1.0f + 0.5f * std::cos(2 * (float)M_PI * b / N)) / N, 0.25f / (1 + b));
    // the CPU chain: the multiply with every product rounded, as nsh_mul_const_vcc
    auto mid = run_cpu({ blocks::fft_vcc::make(N, true, w, shift) }, x, N);
    for (size_t i = 0; i < mid.size(); ++i) mid[i] = cmul(mid[i], k[i % N]);
    const auto ref = run_cpu({ blocks::fft_vcc::make(N, false, w, shift) }, mid, N);

    auto src = blocks::vector_source_c::make(x, false, (unsigned)N);
    auto f1 = hip::fft_vcc::make(N, true, w, shift);
    auto m = hip::multiply_const_vcc::make(k);
    auto f2 = hip::fft_vcc::make(N, false, w, shift);
    auto snk = blocks::vector_sink_c::make(N, frames);
    auto fg = flowgraph::make();
    fg->connect(src, 0, f1, 0)->set_custom_buffer(HIP_BUFFER_ARGS_H2D);
    fg->connect(f1, 0, m, 0)->set_custom_buffer(HIP_BUFFER_ARGS_D2D);
    fg->connect(m, 0, f2, 0)->set_custom_buffer(HIP_BUFFER_ARGS_D2D);
    fg->connect(f2, 0, snk, 0)->set_custom_buffer(HIP_BUFFER_ARGS_D2H);
    auto cpu = schedulers::scheduler_mt::make("cpu", 1u << 18);
    auto gpu = schedulers::scheduler_hip::make("gpu", 0, 1u << 18);
    fg->add_scheduler(cpu);
    fg->add_scheduler(gpu);
    auto da = domain_adapter_direct_conf::make(buffer_preference_t::DOWNSTREAM);
    domain_conf_vec dc{ domain_conf(cpu, { src, snk }, da), domain_conf(gpu, { f1, m, f2 }, da) };
    fg->partition(dc);
    const size_t nfused = gpu->fusion_plan().fused.size();
    fg->run();
    const auto y = snk->data();
    EXPECT_EQ(y.size(), x.size());
    if (y.size() == x.size()) EXPECT_TRUE(close_normwise(y, ref));
    return nfused;
}
TEST(FftHip, PlainChainAt1024StillFuses) { EXPECT_EQ(chain_case(1024, {}, false), (size_t)1); }
TEST(FftHip, WindowedChainIsNotFused) { EXPECT_EQ(chain_case(1024, hann(1024), false), (size_t)0); }
TEST(FftHip, ShiftedChainIsNotFused) { EXPECT_EQ(chain_case(1024, {}, true), (size_t)0); }
TEST(FftHip, ChainAt512IsNotFused) { EXPECT_EQ(chain_case(512, {}, false), (size_t)0); }

// scheduler_hip's per-block kernel timing: one launch per work(), named after the block
TEST(FftHip, KernelTimingNamesTheFftLaunch)
{
    const size_t N = 2048, frames = 200;
    const auto x = synth(N * frames, 9);
    auto blk = hip::fft_vcc::make(N, true, hann(N), true);
    auto r = make_hip({ blk }, x, N);
    r.gpu->set_kernel_timing(true);
    r.fg->run();
    const auto st = r.gpu->kernel_stats();
    size_t found = 0;
    for (auto& k : st) {
        if (k.block.find("fft_vcc") == std::string::npos) continue;
        ++found;
        EXPECT_TRUE(k.launches >= 1);
        EXPECT_EQ(k.items, (uint64_t)frames);
        EXPECT_TRUE(k.kernel_ms > 0);
    }
    EXPECT_EQ(found, (size_t)1);
}
