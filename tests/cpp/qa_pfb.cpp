// pfb_channelizer_ccf through the runtime.
//   PfbCpu.*  the CPU block (it defines the semantics) on scheduler_mt with small buffers, so the
//             stream passes through many work() calls, against an in-test double reference computed
//             from the definition y[m][c] = sum_k h[k] x[mM - k] exp(j 2 pi c k / M).
//   PfbHip.*  the GPU block in a scheduler_hip domain fed from / drained into a scheduler_mt domain
//             over H2D / D2H edges with 64 KiB rings, against the CPU block's output (1e-5
//             norm-wise), restart, a time shard (set_initial_history) and scheduler_hip's per-block
//             kernel timing.
#include "qa.hpp"

#include <cmath>
#include <complex>
#include <stdexcept>
#include <gnuradio/blocklib/blocks/pfb_channelizer_ccf.hpp>
#include <gnuradio/blocklib/blocks/vector_sink.hpp>
#include <gnuradio/blocklib/blocks/vector_source.hpp>
#include <gnuradio/blocklib/hip/pfb_channelizer_ccf.hpp>
#include <gnuradio/domain_adapter_direct.hpp>
#include <gnuradio/flowgraph.hpp>
#include <gnuradio/hip_buffer.hpp>
#include <gnuradio/schedulers/hip/scheduler_hip.hpp>
#include <gnuradio/schedulers/mt/scheduler_mt.hpp>

#include "nsh_hip.h"

using namespace gr;

#include "qa_ref.hpp"

namespace {

// zero initial history; (n / M) items of M channels, time-major
std::vector<gr_complex> pfb_ref(const std::vector<gr_complex>& x, const std::vector<float>& h, int M)
{
    const size_t n_out = x.size() / M;
    std::vector<std::complex<double>> w(M);
    for (int i = 0; i < M; ++i) w[i] = std::polar(1.0, 2.0 * M_PI * i / M);
    std::vector<gr_complex> y(n_out * M);
    for (size_t m = 0; m < n_out; ++m)
        for (int c = 0; c < M; ++c) {
            std::complex<double> acc = 0;
            for (size_t k = 0; k < h.size(); ++k) {
                const long g = (long)(m * M) - (long)k;
                if (g >= 0) acc += (double)h[k] * w[(c * k) % M] * std::complex<double>(x[g]);
            }
            y[m * M + c] = gr_complex(acc);
        }
    return y;
}

// vector_source -> blk -> vector_sink(vlen M) on one scheduler_mt with small buffers; runs twice
std::vector<gr_complex> run_cpu(const block_sptr& blk, const std::vector<gr_complex>& x, int M, bool check_rerun = true)
{
    auto src = blocks::vector_source_c::make(x);
    auto snk = blocks::vector_sink_c::make(M, x.size() / M);
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
// vector_source -[H2D]-> blk -[D2H]-> vector_sink(vlen M): a scheduler_mt domain and a scheduler_hip domain, 64 KiB rings
hip_run make_hip(const block_sptr& blk, const std::vector<gr_complex>& x, int M)
{
    hip_run r;
    auto src = blocks::vector_source_c::make(x);
    r.snk = blocks::vector_sink_c::make(M, x.size() / M);
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
static void pfb_cpu_case(int M, int L)
{
    const size_t n = (size_t)M * (M == 64 ? 700 : 3000) + 1; // the odd input is never consumed
    const auto x = synth(n, 4242);
    const auto h = lowpass(L, 0.4 / M);
    auto blk = blocks::pfb_channelizer_ccf::make(M, h);
    const auto y = run_cpu(blk, x, M);
    EXPECT_EQ(y.size(), (n / M) * M);
    EXPECT_TRUE(close_normwise(y, pfb_ref(x, h, M)));
}
TEST(PfbCpu, M4L48) { pfb_cpu_case(4, 48); }
TEST(PfbCpu, M16L127) { pfb_cpu_case(16, 127); }
TEST(PfbCpu, M64L65) { pfb_cpu_case(64, 65); }

template <class F>
static bool refused(F make)
{
    try {
        make();
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}
TEST(PfbCpu, RefusesBadArguments)
{
    EXPECT_TRUE(refused([] { blocks::pfb_channelizer_ccf::make(12, lowpass(16, 0.1)); }));
    EXPECT_TRUE(refused([] { blocks::pfb_channelizer_ccf::make(128, lowpass(16, 0.1)); }));
    EXPECT_TRUE(refused([] { blocks::pfb_channelizer_ccf::make(4, {}); }));
    EXPECT_TRUE(refused([] { hip::pfb_channelizer_ccf::make(3, lowpass(16, 0.1)); }));
    EXPECT_TRUE(refused([] { hip::pfb_channelizer_ccf::make(2, lowpass(65, 0.1)); }));
    EXPECT_FALSE(refused([] { hip::pfb_channelizer_ccf::make(2, lowpass(64, 0.1)); }));
}

// ---- GPU block ---------------------------------------------------------------------------------
static void pfb_hip_case(int M, int L)
{
    const size_t n = (size_t)M * 9000;
    const auto x = synth(n, 99);
    const auto h = lowpass(L, 0.4 / M);
    const auto ref = run_cpu(blocks::pfb_channelizer_ccf::make(M, h), x, M, false);
    auto blk = hip::pfb_channelizer_ccf::make(M, h);
    auto r = make_hip(blk, x, M);
    r.fg->run();
    const auto y = r.snk->data();
    EXPECT_EQ(y.size(), n);
    EXPECT_TRUE(close_normwise(y, ref));
    std::printf("  M=%d L=%d: %s, %llu launches\n", M, L, blk->kernel().c_str(), (unsigned long long)blk->launches());
    EXPECT_TRUE(blk->launches() > 1);
    r.fg->run(); // history re-armed by start()
    EXPECT_TRUE(r.snk->data() == y || close_normwise(r.snk->data(), ref));
}
TEST(PfbHip, M16L127MatchesCpuAndReruns) { pfb_hip_case(16, 127); }
TEST(PfbHip, M64L200MatchesCpuAndReruns) { pfb_hip_case(64, 200); }

// a time shard: the stream from input n0 on, with the L-1 raw samples before it as initial history,
// gives the tail of the whole stream's output
TEST(PfbHip, TimeShardReproducesTail)
{
    const int M = 8, L = 63;
    const size_t n = (size_t)M * 30000, n0 = (size_t)M * 12345;
    const auto x = synth(n, 31);
    const auto h = lowpass(L, 0.05);
    auto whole = hip::pfb_channelizer_ccf::make(M, h);
    auto rw = make_hip(whole, x, M);
    rw.fg->run();
    const auto yw = rw.snk->data();
    ASSERT_TRUE(yw.size() == n);

    auto shard = hip::pfb_channelizer_ccf::make(M, h);
    shard->set_initial_history(std::vector<gr_complex>(x.begin() + (n0 - (L - 1)), x.begin() + n0));
    auto rs = make_hip(shard, std::vector<gr_complex>(x.begin() + n0, x.end()), M);
    rs.fg->run();
    const auto ys = rs.snk->data();
    EXPECT_TRUE(close_normwise(ys, std::vector<gr_complex>(yw.begin() + n0, yw.end())));
    // without the history the shard's first items differ
    auto cold = hip::pfb_channelizer_ccf::make(M, h);
    auto rc = make_hip(cold, std::vector<gr_complex>(x.begin() + n0, x.end()), M);
    rc.fg->run();
    const auto yc = rc.snk->data();
    ASSERT_TRUE(yc.size() == ys.size());
    double d = 0;
    for (size_t i = 0; i < (size_t)M * 4; ++i) d = std::max(d, (double)std::abs(ys[i] - yc[i]));
    EXPECT_TRUE(d > 1e-3);
}

// scheduler_hip's per-block kernel timing needs nothing from the block: one nsh::launch per work()
TEST(PfbHip, KernelTimingOneLaunchPerWork)
{
    const int M = 16;
    const size_t n = (size_t)M * 20000;
    const auto x = synth(n, 8);
    auto blk = hip::pfb_channelizer_ccf::make(M, lowpass(127, 0.02));
    auto r = make_hip(blk, x, M);
    r.gpu->set_kernel_timing(true);
    r.fg->run();
    const auto st = r.gpu->kernel_stats();
    size_t found = 0;
    for (auto& k : st) {
        if (k.block.find("pfb_channelizer_ccf") == std::string::npos) continue;
        ++found;
        EXPECT_EQ(k.launches, blk->launches());
        EXPECT_EQ(k.items, (uint64_t)(n / M));
        EXPECT_TRUE(k.kernel_ms > 0);
    }
    EXPECT_EQ(found, (size_t)1);
}
