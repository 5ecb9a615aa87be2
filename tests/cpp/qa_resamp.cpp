// rational_resampler_ccf through the runtime.
//   ResampCpu.*  the CPU block (it defines the semantics) on scheduler_mt with 8 KiB buffers, so the
//                stream passes through many work() calls, against an in-test double reference computed
//                from the definition y[n] = sum_k h[k] u[nD - k], u the input zero-stuffed by I.
//   ResampHip.*  the GPU block in a scheduler_hip domain fed from / drained into a scheduler_mt domain
//                over H2D / D2H edges with 64 KiB rings, against the CPU block's output (1e-5
//                norm-wise), restart, a time shard (set_initial_history) and scheduler_hip's per-block
//                kernel timing.
#include "qa.hpp"

#include <cmath>
#include <complex>
#include <stdexcept>
#include <gnuradio/blocklib/blocks/rational_resampler_ccf.hpp>
#include <gnuradio/blocklib/blocks/vector_sink.hpp>
#include <gnuradio/blocklib/blocks/vector_source.hpp>
#include <gnuradio/blocklib/hip/rational_resampler_ccf.hpp>
#include <gnuradio/domain_adapter_direct.hpp>
#include <gnuradio/flowgraph.hpp>
#include <gnuradio/hip_buffer.hpp>
#include <gnuradio/schedulers/hip/scheduler_hip.hpp>
#include <gnuradio/schedulers/mt/scheduler_mt.hpp>

#include "nsh_hip.h"

using namespace gr;

#include "qa_ref.hpp"

namespace {

// zero initial history; floor(n / D) units of I outputs
std::vector<gr_complex> resamp_ref(const std::vector<gr_complex>& x, const std::vector<float>& h, int I, int D)
{
    const size_t n_out = x.size() / D * I;
    std::vector<gr_complex> y(n_out);
    for (size_t n = 0; n < n_out; ++n) {
        std::complex<double> acc = 0;
        for (size_t k = (n * D) % I; k < h.size(); k += I) { // u[nD - k] = x[(nD - k) / I]
            const long j = ((long)(n * D) - (long)k) / I;
            if ((long)(n * D) >= (long)k) acc += (double)h[k] * std::complex<double>(x[j]);
        }
        y[n] = gr_complex(acc);
    }
    return y;
}

// a low-pass for resampling by I / D with the interpolator's gain I
std::vector<float> resamp_taps(int L, int I, int D)
{
    if (L == 1) return { (float)I };
    auto h = lowpass(L, 0.4 / std::max(I, D));
    for (auto& v : h) v *= (float)I;
    return h;
}

// vector_source -> blk -> vector_sink on one scheduler_mt with 8 KiB buffers; runs twice
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

// ---- CPU block ---------------------------------------------------------------------------------
// n inputs give exactly floor(n / D) I outputs: the leftover shorter than D is never consumed
static void resamp_cpu_case(int I, int D, int L, size_t n)
{
    const auto x = synth(n, 4242);
    const auto h = resamp_taps(L, I, D);
    auto blk = blocks::rational_resampler_ccf::make(I, D, h);
    const auto y = run_cpu(blk, x);
    EXPECT_EQ(y.size(), n / D * I);
    EXPECT_TRUE(close_normwise(y, resamp_ref(x, h, I, D)));
}
TEST(ResampCpu, I3D2L95) { resamp_cpu_case(3, 2, 95, 20001); }
TEST(ResampCpu, I4D5L159NotDividingTheRing) { resamp_cpu_case(4, 5, 159, 5 * 4000 + 3); }
TEST(ResampCpu, I2D7L30) { resamp_cpu_case(2, 7, 30, 7 * 3000 + 6); }
TEST(ResampCpu, I64D1L1024SmallBuffers) { resamp_cpu_case(64, 1, 1024, 1500); }
TEST(ResampCpu, I1D64L1024SmallBuffers) { resamp_cpu_case(1, 64, 1024, 64 * 300 + 63); }
TEST(ResampCpu, I5D3SingleTap) { resamp_cpu_case(5, 3, 1, 3 * 2000 + 1); }

template <class F>
static std::string refusal(F make)
{
    try {
        make();
    } catch (const std::invalid_argument& e) {
        return e.what();
    }
    return "";
}
TEST(ResampCpu, RefusesBadArguments)
{
    const std::vector<float> h(16, 0.1f);
    // both blocks refuse what the plan refuses, with its words
    EXPECT_EQ(refusal([&] { blocks::rational_resampler_ccf::make(0, 1, h); }),
              std::string("rational_resampler_ccf: interpolation must be in [1, 64]"));
    EXPECT_EQ(refusal([&] { blocks::rational_resampler_ccf::make(1, 65, h); }),
              std::string("rational_resampler_ccf: decimation must be in [1, 64]"));
    EXPECT_EQ(refusal([&] { blocks::rational_resampler_ccf::make(1, 1, {}); }),
              std::string("rational_resampler_ccf: ntaps must be in [1, 1024]"));
    EXPECT_EQ(refusal([&] { hip::rational_resampler_ccf::make(65, 1, h); }),
              std::string("hip::rational_resampler_ccf: interpolation must be in [1, 64]"));
    EXPECT_EQ(refusal([&] { hip::rational_resampler_ccf::make(1, 0, h); }),
              std::string("hip::rational_resampler_ccf: decimation must be in [1, 64]"));
    EXPECT_EQ(refusal([&] { hip::rational_resampler_ccf::make(1, 1, std::vector<float>(1025, 0.f)); }),
              std::string("hip::rational_resampler_ccf: ntaps must be in [1, 1024]"));
    EXPECT_EQ(refusal([&] { hip::rational_resampler_ccf::make(64, 64, std::vector<float>(1024, 0.f)); }), std::string(""));
}

// ---- GPU block ---------------------------------------------------------------------------------
static void resamp_hip_case(int I, int D, int L, size_t units)
{
    const size_t n = (size_t)D * units;
    const auto x = synth(n, 99);
    const auto h = resamp_taps(L, I, D);
    const auto ref = run_cpu(blocks::rational_resampler_ccf::make(I, D, h), x, false);
    auto blk = hip::rational_resampler_ccf::make(I, D, h);
    auto r = make_hip(blk, x);
    r.fg->run();
    const auto y = r.snk->data();
    EXPECT_EQ(y.size(), units * I);
    EXPECT_TRUE(close_normwise(y, ref));
    std::printf("  I=%d D=%d L=%d: %s, %llu launches\n", I, D, L, blk->kernel().c_str(), (unsigned long long)blk->launches());
    EXPECT_TRUE(blk->launches() > 1);
    r.fg->run(); // a second start() begins from a clean history
    EXPECT_TRUE(r.snk->data() == y);
}
TEST(ResampHip, I3D2L95MatchesCpuAndReruns) { resamp_hip_case(3, 2, 95, 30000); }
TEST(ResampHip, I4D5L159MatchesCpuAndReruns) { resamp_hip_case(4, 5, 159, 12000); }
TEST(ResampHip, I64D1L1024MatchesCpuAndReruns) { resamp_hip_case(64, 1, 1024, 3000); }
TEST(ResampHip, I1D64L1024MatchesCpuAndReruns) { resamp_hip_case(1, 64, 1024, 1500); }

// a time shard: the stream from input n0 (a multiple of D) on, with the Q-1 raw samples before it as
// initial history, gives the tail of the whole stream's output
TEST(ResampHip, TimeShardReproducesTail)
{
    const int I = 3, D = 5, L = 95, H = (L + I - 1) / I - 1;
    const size_t n = (size_t)D * 30000, n0 = (size_t)D * 12345;
    const auto x = synth(n, 31);
    const auto h = resamp_taps(L, I, D);
    auto whole = hip::rational_resampler_ccf::make(I, D, h);
    auto rw = make_hip(whole, x);
    rw.fg->run();
    const auto yw = rw.snk->data();
    ASSERT_TRUE(yw.size() == n / D * I);

    auto shard = hip::rational_resampler_ccf::make(I, D, h);
    shard->set_initial_history(std::vector<gr_complex>(x.begin() + (n0 - H), x.begin() + n0));
    auto rs = make_hip(shard, std::vector<gr_complex>(x.begin() + n0, x.end()));
    rs.fg->run();
    const auto ys = rs.snk->data();
    // bit for bit: an output's sum does not depend on the call it falls into
    EXPECT_TRUE(ys == std::vector<gr_complex>(yw.begin() + n0 / D * I, yw.end()));
    // without the history the shard's first outputs differ
    auto cold = hip::rational_resampler_ccf::make(I, D, h);
    auto rc = make_hip(cold, std::vector<gr_complex>(x.begin() + n0, x.end()));
    rc.fg->run();
    const auto yc = rc.snk->data();
    ASSERT_TRUE(yc.size() == ys.size());
    double d = 0;
    for (size_t i = 0; i < (size_t)I * 4; ++i) d = std::max(d, (double)std::abs(ys[i] - yc[i]));
    EXPECT_TRUE(d > 1e-3);
}

// scheduler_hip's per-block kernel timing needs nothing from the block: one nsh::launch per work()
TEST(ResampHip, KernelTimingOneLaunchPerWork)
{
    const int I = 4, D = 5;
    const size_t n = (size_t)D * 20000;
    const auto x = synth(n, 8);
    auto blk = hip::rational_resampler_ccf::make(I, D, resamp_taps(159, I, D));
    auto r = make_hip(blk, x);
    r.gpu->set_kernel_timing(true);
    r.fg->run();
    const auto st = r.gpu->kernel_stats();
    size_t found = 0;
    for (auto& k : st) {
        if (k.block.find("rational_resampler_ccf") == std::string::npos) continue;
        ++found;
        EXPECT_EQ(k.launches, blk->launches());
        EXPECT_EQ(k.items, (uint64_t)(n / D * I));
        EXPECT_TRUE(k.kernel_ms > 0);
    }
    EXPECT_EQ(found, (size_t)1);
}
