// Stream tags through the scheduler (reference schedulers/mt/test/qa_tags.cpp:21-220,
// restated with the same flowgraphs and expected tag counts; its t5 is disabled there), plus
// the same propagation across device edges: H2D / D2D / D2H hip_buffers and gr::hip blocks
// keep _total_read/_total_written exact, so tag offsets survive the GPU domain.
//
// HostRateTags / DeviceRateTags: tags through every rate-changing block, CPU and gr::hip. A tag
// follows its item (buffer::propagate_tags): through a fixed I:D block a tag at source offset t
// lands at floor(t I / D), however the stream is cut into work() calls. Every test compares the
// complete list of (sequence number, offset) pairs the sink annotator saw with that closed form.
// (main() selects cases by substring, so neither suite's name may contain the other's.)
#include "qa.hpp"

#include <cmath>
#include <cstring>
#include <gnuradio/blocklib/blocks/annotator.hpp>
#include <gnuradio/blocklib/blocks/arith.hpp>
#include <gnuradio/blocklib/blocks/copy.hpp>
#include <gnuradio/blocklib/blocks/fft_filter.hpp>
#include <gnuradio/blocklib/blocks/fir_filter_ccf.hpp>
#include <gnuradio/blocklib/blocks/freq_xlating_fft_filter_ccc.hpp>
#include <gnuradio/blocklib/blocks/freq_xlating_fir_filter_ccf.hpp>
#include <gnuradio/blocklib/blocks/head.hpp>
#include <gnuradio/blocklib/blocks/null_sink.hpp>
#include <gnuradio/blocklib/blocks/null_source.hpp>
#include <gnuradio/blocklib/blocks/pfb_arb_resampler_ccf.hpp>
#include <gnuradio/blocklib/blocks/pfb_channelizer_ccf.hpp>
#include <gnuradio/blocklib/blocks/pfb_synthesizer_ccf.hpp>
#include <gnuradio/blocklib/blocks/psd.hpp>
#include <gnuradio/blocklib/blocks/rational_resampler_ccf.hpp>
#include <gnuradio/blocklib/blocks/vector_source.hpp>
#include <gnuradio/blocklib/hip/copy.hpp>
#include <gnuradio/blocklib/hip/fft.hpp>
#include <gnuradio/blocklib/hip/fft_filter.hpp>
#include <gnuradio/blocklib/hip/fir_filter_cascade_ccf.hpp>
#include <gnuradio/blocklib/hip/fir_filter_ccf.hpp>
#include <gnuradio/blocklib/hip/freq_xlating_fft_filter_ccc.hpp>
#include <gnuradio/blocklib/hip/freq_xlating_fir_filter_ccf.hpp>
#include <gnuradio/blocklib/hip/multiply_const.hpp>
#include <gnuradio/blocklib/hip/pfb_arb_resampler_ccf.hpp>
#include <gnuradio/blocklib/hip/pfb_channelizer_ccf.hpp>
#include <gnuradio/blocklib/hip/pfb_synthesizer_ccf.hpp>
#include <gnuradio/blocklib/hip/psd.hpp>
#include <gnuradio/blocklib/hip/rational_resampler_ccf.hpp>
#include <gnuradio/domain_adapter_direct.hpp>
#include <gnuradio/flowgraph.hpp>
#include <gnuradio/hip_buffer.hpp>
#include <gnuradio/schedulers/hip/scheduler_hip.hpp>
#include <gnuradio/schedulers/mt/scheduler_mt.hpp>

using namespace gr;

#include "qa_ref.hpp"

using A = blocks::annotator;
constexpr auto ONE = tag_propagation_policy_t::TPP_ONE_TO_ONE;
constexpr auto ALL = tag_propagation_policy_t::TPP_ALL_TO_ALL;

TEST(SchedulerMTTags, OneToOne)
{
    const int N = 40000;
    auto fg = flowgraph::make();
    auto src = blocks::null_source::make(sizeof(int));
    auto head = blocks::head::make(sizeof(int), N);
    auto ann0 = A::make(10000, sizeof(int), 1, 2, ONE);
    auto ann1 = A::make(10000, sizeof(int), 1, 1, ONE);
    auto ann2 = A::make(10000, sizeof(int), 1, 1, ONE);
    auto snk0 = blocks::null_sink::make(sizeof(int));
    auto snk1 = blocks::null_sink::make(sizeof(int));
    fg->connect(src, 0, head, 0);
    fg->connect(head, 0, ann0, 0);
    fg->connect(ann0, 0, ann1, 0);
    fg->connect(ann0, 1, ann2, 0);
    fg->connect(ann1, 0, snk0, 0);
    fg->connect(ann2, 0, snk1, 0);
    fg->set_scheduler(schedulers::scheduler_mt::make());
    fg->validate();
    fg->start();
    fg->wait();
    EXPECT_EQ(ann0->data().size(), 0u);
    EXPECT_EQ(ann1->data().size(), 4u);
    EXPECT_EQ(ann2->data().size(), 4u);
}

TEST(SchedulerMTTags, t1)
{
    const int N = 40000;
    auto fg = flowgraph::make();
    auto src = blocks::null_source::make(sizeof(int));
    auto head = blocks::head::make(sizeof(int), N);
    auto ann0 = A::make(10000, sizeof(int), 1, 2, ALL);
    auto ann1 = A::make(10000, sizeof(int), 1, 1, ALL);
    auto ann2 = A::make(10000, sizeof(int), 1, 1, ALL);
    auto ann3 = A::make(10000, sizeof(int), 1, 1, ALL);
    auto ann4 = A::make(10000, sizeof(int), 1, 1, ALL);
    auto snk0 = blocks::null_sink::make(sizeof(int));
    auto snk1 = blocks::null_sink::make(sizeof(int));
    fg->connect(src, 0, head, 0);
    fg->connect(head, 0, ann0, 0);
    fg->connect(ann0, 0, ann1, 0);
    fg->connect(ann0, 1, ann2, 0);
    fg->connect(ann1, 0, ann3, 0);
    fg->connect(ann2, 0, ann4, 0);
    fg->connect(ann3, 0, snk0, 0);
    fg->connect(ann4, 0, snk1, 0);
    fg->set_scheduler(schedulers::scheduler_mt::make());
    fg->validate();
    fg->run();
    EXPECT_EQ(ann0->data().size(), 0u);
    EXPECT_EQ(ann3->data().size(), 8u);
    EXPECT_EQ(ann4->data().size(), 8u);
}

TEST(SchedulerMTTags, t2)
{
    const int N = 40000;
    auto fg = flowgraph::make();
    auto src = blocks::null_source::make(sizeof(int));
    auto head = blocks::head::make(sizeof(int), N);
    auto ann0 = A::make(10000, sizeof(int), 1, 2, ALL);
    auto ann1 = A::make(10000, sizeof(int), 2, 3, ALL);
    auto ann2 = A::make(10000, sizeof(int), 1, 1, ALL);
    auto ann3 = A::make(10000, sizeof(int), 1, 1, ALL);
    auto ann4 = A::make(10000, sizeof(int), 1, 1, ALL);
    auto snk0 = blocks::null_sink::make(sizeof(int));
    auto snk1 = blocks::null_sink::make(sizeof(int));
    auto snk2 = blocks::null_sink::make(sizeof(int));
    fg->connect(src, 0, head, 0);
    fg->connect(head, 0, ann0, 0);
    fg->connect(ann0, 0, ann1, 0);
    fg->connect(ann0, 1, ann1, 1);
    fg->connect(ann1, 0, ann2, 0);
    fg->connect(ann1, 1, ann3, 0);
    fg->connect(ann1, 2, ann4, 0);
    fg->connect(ann2, 0, snk0, 0);
    fg->connect(ann3, 0, snk1, 0);
    fg->connect(ann4, 0, snk2, 0);
    fg->set_scheduler(schedulers::scheduler_mt::make());
    fg->validate();
    fg->run();
    EXPECT_EQ(ann0->data().size(), 0u);
    EXPECT_EQ(ann1->data().size(), 8u);
    EXPECT_EQ(ann2->data().size(), 12u);
    EXPECT_EQ(ann3->data().size(), 12u);
    EXPECT_EQ(ann4->data().size(), 12u);
}

TEST(SchedulerMTTags, t3)
{
    const int N = 40000;
    auto fg = flowgraph::make();
    auto src = blocks::null_source::make(sizeof(int));
    auto head = blocks::head::make(sizeof(int), N);
    auto ann0 = A::make(10000, sizeof(int), 2, 2, ONE);
    auto ann1 = A::make(10000, sizeof(int), 1, 1, ALL);
    auto ann2 = A::make(10000, sizeof(int), 1, 1, ALL);
    auto ann3 = A::make(10000, sizeof(int), 1, 1, ONE);
    auto ann4 = A::make(10000, sizeof(int), 1, 1, ONE);
    auto snk0 = blocks::null_sink::make(sizeof(int));
    auto snk1 = blocks::null_sink::make(sizeof(int));
    fg->connect(src, 0, head, 0);
    fg->connect(head, 0, ann0, 0);
    fg->connect(head, 0, ann0, 1);
    fg->connect(ann0, 0, ann1, 0);
    fg->connect(ann0, 1, ann2, 0);
    fg->connect(ann1, 0, ann3, 0);
    fg->connect(ann2, 0, ann4, 0);
    fg->connect(ann3, 0, snk0, 0);
    fg->connect(ann4, 0, snk1, 0);
    auto sched = schedulers::scheduler_mt::make();
    sched->add_block_group({ src, head, ann0, ann1, ann2, ann3, ann4, snk0, snk1 });
    fg->set_scheduler(sched);
    fg->validate();
    fg->start();
    fg->wait();
    EXPECT_EQ(ann0->data().size(), 0u);
    EXPECT_EQ(ann3->data().size(), 8u);
    EXPECT_EQ(ann4->data().size(), 8u);
}

// Not in the reference (its domain adapters carry no tags): tags crossing in-process domain
// boundaries. src -> head -> ann0 | copy | ann1 -> sink in three scheduler_mt domains;
// the adapter pair's tag calls resolve to the shared edge buffer, so ann1 sees ann0's 4 tags
// at their absolute offsets.
TEST(SchedulerMTTags, AcrossDomains)
{
    const int N = 40000;
    auto fg = flowgraph::make();
    auto src = blocks::null_source::make(sizeof(gr_complex));
    auto head = blocks::head::make(sizeof(gr_complex), N);
    auto ann0 = A::make(10000, sizeof(gr_complex), 1, 1, ALL);
    auto cp = blocks::copy::make(sizeof(gr_complex));
    auto ann1 = A::make(1u << 30, sizeof(gr_complex), 1, 1, ALL);
    auto snk = blocks::null_sink::make(sizeof(gr_complex));
    fg->connect(src, 0, head, 0);
    fg->connect(head, 0, ann0, 0);
    fg->connect(ann0, 0, cp, 0);
    fg->connect(cp, 0, ann1, 0);
    fg->connect(ann1, 0, snk, 0);
    auto a = schedulers::scheduler_mt::make("a", 32768);
    auto b = schedulers::scheduler_mt::make("b", 32768);
    auto a2 = schedulers::scheduler_mt::make("c", 32768);
    fg->add_scheduler(a);
    fg->add_scheduler(b);
    fg->add_scheduler(a2);
    auto da = domain_adapter_direct_conf::make(buffer_preference_t::DOWNSTREAM);
    // crossings ann0 -> cp (the annotator writes into an adapter: offsets come from the
    // edge buffer's counters) and cp -> ann1
    domain_conf_vec dc{ domain_conf(a, { src, head, ann0 }, da), domain_conf(b, { cp }, da),
                        domain_conf(a2, { ann1, snk }, da) };
    fg->partition(dc);
    fg->run();
    auto seen = ann1->data();
    ASSERT_TRUE(seen.size() == 4u);
    for (size_t i = 0; i < 4; ++i) {
        EXPECT_EQ(seen[i].offset, (uint64_t)(10000 * i));
        EXPECT_TRUE(std::get<int64_t>(seen[i].value->value()) == (int64_t)i);
    }
}

// Device edges: annotator -[H2D]-> hip::copy -[D2D]-> hip::copy -[D2H]-> annotator. The
// second annotator must see the first one's 4 tags at their original absolute offsets.
TEST(DeviceTags, ThroughHipBlocks)
{
    const int N = 40000;
    auto fg = flowgraph::make();
    auto src = blocks::null_source::make(sizeof(gr_complex));
    auto head = blocks::head::make(sizeof(gr_complex), N);
    auto ann0 = A::make(10000, sizeof(gr_complex), 1, 1, ALL);
    auto c1 = hip::copy::make(1);
    auto c2 = hip::copy::make(1);
    auto ann1 = A::make(1u << 30, sizeof(gr_complex), 1, 1, ALL);
    auto snk = blocks::null_sink::make(sizeof(gr_complex));
    fg->connect(src, 0, head, 0);
    fg->connect(head, 0, ann0, 0);
    fg->connect(ann0, 0, c1, 0)->set_custom_buffer(HIP_BUFFER_ARGS_H2D);
    fg->connect(c1, 0, c2, 0)->set_custom_buffer(HIP_BUFFER_ARGS_D2D);
    fg->connect(c2, 0, ann1, 0)->set_custom_buffer(HIP_BUFFER_ARGS_D2H);
    fg->connect(ann1, 0, snk, 0);
    fg->set_scheduler(schedulers::scheduler_mt::make("mt", 32768));
    fg->validate();
    fg->run();
    auto seen = ann1->data();
    // ann1 tags offset 0 itself (when = 2^30), which it does not see on its input
    ASSERT_TRUE(seen.size() == 4u);
    for (size_t i = 0; i < seen.size(); ++i) {
        EXPECT_EQ(seen[i].offset, (uint64_t)(10000 * i));
        EXPECT_TRUE(std::get<int64_t>(seen[i].value->value()) == (int64_t)i);
    }
}

// The same through scheduler_hip with elementwise fusion: CPU domain (annotators) and a GPU
// domain where copy -> multiply_const(1) -> copy is fused into one block. Tags must keep
// their absolute offsets through the fused block.
TEST(DeviceTags, ThroughFusedChain)
{
    const int N = 40000;
    auto fg = flowgraph::make();
    auto src = blocks::null_source::make(sizeof(gr_complex));
    auto head = blocks::head::make(sizeof(gr_complex), N);
    auto ann0 = A::make(10000, sizeof(gr_complex), 1, 1, ALL);
    auto c1 = hip::copy::make(1);
    auto m = hip::multiply_const_cc::make(gr_complex(1.0f, 0.0f));
    auto c2 = hip::copy::make(1);
    auto ann1 = A::make(1u << 30, sizeof(gr_complex), 1, 1, ALL);
    auto snk = blocks::null_sink::make(sizeof(gr_complex));
    fg->connect(src, 0, head, 0);
    fg->connect(head, 0, ann0, 0);
    fg->connect(ann0, 0, c1, 0)->set_custom_buffer(HIP_BUFFER_ARGS_H2D);
    fg->connect(c1, 0, m, 0);
    fg->connect(m, 0, c2, 0);
    fg->connect(c2, 0, ann1, 0)->set_custom_buffer(HIP_BUFFER_ARGS_D2H);
    fg->connect(ann1, 0, snk, 0);
    auto cpu = schedulers::scheduler_mt::make("cpu", 32768);
    auto gpu = schedulers::scheduler_hip::make("gpu", 0, 1u << 16);
    fg->add_scheduler(cpu);
    fg->add_scheduler(gpu);
    auto da = domain_adapter_direct_conf::make(buffer_preference_t::DOWNSTREAM);
    domain_conf_vec dc{ domain_conf(cpu, { src, head, ann0, ann1, snk }, da), domain_conf(gpu, { c1, m, c2 }, da) };
    fg->partition(dc);
    ASSERT_TRUE(gpu->fusion_plan().fused.size() == 1u);
    fg->run();
    auto seen = ann1->data();
    ASSERT_TRUE(seen.size() == 4u);
    for (size_t i = 0; i < seen.size(); ++i) {
        EXPECT_EQ(seen[i].offset, (uint64_t)(10000 * i));
        EXPECT_TRUE(std::get<int64_t>(seen[i].value->value()) == (int64_t)i);
    }
}

// ---- tags through rate-changing blocks -------------------------------------------------------------
namespace {

constexpr auto DONT = tag_propagation_policy_t::TPP_DONT;
constexpr size_t CSZ = sizeof(gr_complex);
using pairs = std::vector<std::pair<int64_t, uint64_t>>; // (sequence number, offset), in the order seen
using maker = std::function<block_sptr()>;

pairs pairs_of(const A::sptr& a, size_t from = 0)
{
    const auto seen = a->data();
    pairs r;
    for (size_t i = from; i < seen.size(); ++i) r.emplace_back(std::get<int64_t>(seen[i].value->value()), seen[i].offset);
    return r;
}

// The closed form. The source annotator tags every `when`-th item: sequence number t / when at
// offset t. The I:D block under test started with its input read up to r0 and its output written
// up to w0, and consumed the n_in / D whole units of the n_in items that followed.
pairs closed_form(uint64_t when, uint64_t n_in, uint64_t I, uint64_t D, uint64_t r0 = 0, uint64_t w0 = 0)
{
    pairs r;
    const uint64_t end = r0 + n_in / D * D;
    for (uint64_t t = (r0 + when - 1) / when * when; t < end; t += when) r.emplace_back((int64_t)(t / when), w0 + (t - r0) * I / D);
    return r;
}

// the complete lists must be equal; one line names the first difference
bool same(const pairs& got, const pairs& want, const std::string& what)
{
    if (got == want) return true;
    size_t i = 0;
    while (i < got.size() && i < want.size() && got[i] == want[i]) ++i;
    auto show = [i](const pairs& p) {
        return i < p.size() ? "(" + std::to_string(p[i].first) + ", " + std::to_string(p[i].second) + ")" : std::string("nothing");
    };
    std::fprintf(stderr, "  %s: saw %zu tags, expected %zu; first difference at entry %zu: saw %s, expected %s\n", what.c_str(),
                 got.size(), want.size(), i, show(got).c_str(), show(want).c_str());
    return false;
}

std::string label(const char* what, uint64_t when, unsigned buf)
{
    return std::string(what) + " when=" + std::to_string(when) + " buf=" + std::to_string(buf);
}

std::vector<gr_complex> complex_taps(const std::vector<float>& h)
{
    std::vector<gr_complex> c(h.size());
    for (size_t i = 0; i < h.size(); ++i) c[i] = gr_complex(h[i], 0.25f * h[i]);
    return c;
}

struct tagged_graph {
    flowgraph_sptr fg;
    A::sptr sink;
    blocks::null_sink::sptr snk;
};
// null_source -> head(n) -> annotator(when) -> blk -> annotator(2^30) -> null_sink, no scheduler yet;
// device_edges: H2D into blk and D2H out of it
tagged_graph tagged(const block_sptr& blk, size_t in_item, size_t out_item, uint64_t when, size_t n, bool device_edges = false)
{
    tagged_graph g;
    g.fg = flowgraph::make();
    auto src = blocks::null_source::make(in_item);
    auto head = blocks::head::make(in_item, n);
    auto ann0 = A::make(when, in_item, 1, 1, ALL);
    g.sink = A::make(1u << 30, out_item, 1, 1, ALL);
    g.snk = blocks::null_sink::make(out_item);
    g.fg->connect(src, 0, head, 0);
    g.fg->connect(head, 0, ann0, 0);
    auto e_in = g.fg->connect(ann0, 0, blk, 0);
    auto e_out = g.fg->connect(blk, 0, g.sink, 0);
    if (device_edges) {
        e_in->set_custom_buffer(HIP_BUFFER_ARGS_H2D);
        e_out->set_custom_buffer(HIP_BUFFER_ARGS_D2H);
    }
    g.fg->connect(g.sink, 0, g.snk, 0);
    return g;
}

tagged_graph run_on_mt(const block_sptr& blk, size_t in_item, size_t out_item, uint64_t when, size_t n, unsigned buf,
                       bool device_edges = false)
{
    auto g = tagged(blk, in_item, out_item, when, n, device_edges);
    g.fg->set_scheduler(schedulers::scheduler_mt::make("mt", buf));
    g.fg->validate();
    g.fg->run();
    return g;
}

// A fixed I:D block on scheduler_mt: a prime spacing (offsets are multiples of no D) and a tag on
// every item (D tags on each output item, or every I-th output tagged; none lost, none twice), with
// 4096-byte buffers (many work() calls) and 1 MiB ones (few): identical lists, equal to the closed form.
void host_case(const char* what, const maker& make, size_t in_item, size_t out_item, uint64_t I, uint64_t D, size_t n)
{
    for (uint64_t when : { (uint64_t)997, (uint64_t)1 }) {
        const pairs want = closed_form(when, n, I, D);
        pairs small;
        for (unsigned buf : { 4096u, 1u << 20 }) {
            const pairs got = pairs_of(run_on_mt(make(), in_item, out_item, when, n, buf).sink);
            EXPECT_TRUE(same(got, want, label(what, when, buf)));
            if (buf == 4096u)
                small = got;
            else
                EXPECT_TRUE(got == small);
        }
    }
}

// The same for a gr::hip block between an H2D and a D2H edge, as DeviceTags.ThroughHipBlocks.
void device_case(const char* what, const maker& make, size_t in_item, size_t out_item, uint64_t I, uint64_t D, size_t n)
{
    for (uint64_t when : { (uint64_t)997, (uint64_t)1 }) {
        const pairs got = pairs_of(run_on_mt(make(), in_item, out_item, when, n, 32768, true).sink);
        EXPECT_TRUE(same(got, closed_form(when, n, I, D), label(what, when, 32768)));
    }
}

// pfb_arb_resampler_ccf sets its own consumed and produced counts: no closed form, but the rule
// bounds where a tag lands. Count in output items and let q be the block's phase when a call
// starts (how far its next output W lies past its first unread input R) and q' the phase when it
// ends: the call's counts obey p = c r + q' - q exactly. A tag on input R + k goes to
// W + floor(k p / c), its exact image is W - q + k r, so
//     offset - t r = q (1 - k/c) + q' k/c - f,   0 <= f < 1   (the per-call floor),
// which lies between min(q, q') - 1 and max(q, q'); with p == 0 the tag goes to W and q = c r + q',
// the same bounds. nsh_arb::span_of leaves the next output less than one input item or one output
// item ahead, q < max(r, 1), and the first tag (t = 0: R = W = k = q = 0) has deviation 0. So every
// deviation lies in (-1, max(r, 1)), for r <= 1.37 well within the +-3 asserted; the step's
// rounding (r is round(F 2^32 / r) inverted, below 2^-27 relative) moves it by less than 0.001 here.
// Exactly once and in order: the sequence numbers seen are 0, 1, 2, ... without a gap; none lost:
// the first tag not seen has its image within 3 items of the end of the produced stream or beyond.
void check_arb(const pairs& got, uint64_t when, double rate, uint64_t n_in, uint64_t n_out, const std::string& what)
{
    bool once = true, ordered = true, inside = true;
    double worst = 0;
    for (size_t i = 0; i < got.size(); ++i) {
        once = once && got[i].first == (int64_t)i;
        ordered = ordered && (i == 0 || got[i].second >= got[i - 1].second);
        inside = inside && got[i].second < n_out;
        const double dev = (double)got[i].second - (double)(got[i].first * (int64_t)when) * rate - (double)got[0].second;
        if (std::fabs(dev) > std::fabs(worst)) worst = dev;
    }
    const uint64_t t_next = (uint64_t)got.size() * when;
    std::printf("  %s: %zu tags on %llu outputs, worst deviation from the first tag's %+.3f items\n", what.c_str(), got.size(),
                (unsigned long long)n_out, worst);
    EXPECT_TRUE(!got.empty());
    EXPECT_TRUE(once);
    EXPECT_TRUE(ordered);
    EXPECT_TRUE(inside);
    EXPECT_TRUE(t_next >= n_in || (double)t_next * rate + 3.0 >= (double)n_out);
    EXPECT_TRUE(std::fabs(worst) <= 3.0);
}

// the prototype of an arbitrary resampler with F filters: gain F, cut-off inside both Nyquist bands
std::vector<float> arb_taps(int L, int F, double rate)
{
    auto h = lowpass(L, 0.4 / F * std::min(1.0, rate));
    for (auto& v : h) v *= (float)F;
    return h;
}

void host_arb_case(double rate)
{
    const size_t n = 100003;
    for (uint64_t when : { (uint64_t)997, (uint64_t)1 })
        for (unsigned buf : { 4096u, 1u << 20 }) {
            auto g = run_on_mt(blocks::pfb_arb_resampler_ccf::make(rate, arb_taps(256, 32, rate), 32), CSZ, CSZ, when, n, buf);
            check_arb(pairs_of(g.sink), when, rate, n, g.snk->consumed(), label("pfb_arb_resampler_ccf", when, buf));
        }
}

// passes at most `chunk` items per work(): the block behind it sees its stream a few items at a time
class trickle : public block
{
public:
    static std::shared_ptr<trickle> make(int chunk)
    {
        auto p = std::make_shared<trickle>(chunk);
        p->add_port(port<gr_complex>::make("in", port_direction_t::INPUT));
        p->add_port(port<gr_complex>::make("out", port_direction_t::OUTPUT));
        return p;
    }
    explicit trickle(int chunk) : block("trickle"), _chunk(chunk) {}
    work_return_code_t work(std::vector<block_work_input>& in, std::vector<block_work_output>& out) override
    {
        const int n = std::min(std::min(in[0].n_items, out[0].n_items), _chunk);
        std::memcpy(out[0].buffer->write_ptr(), in[0].buffer->read_ptr(), (size_t)n * sizeof(gr_complex));
        in[0].n_consumed = n;
        out[0].n_produced = n;
        return work_return_code_t::WORK_OK;
    }

private:
    int _chunk;
};

} // namespace

// ---- 1: the decimating FIR; D = 1 pins that nothing changed for a 1:1 block ------------------------
static void host_fir_case(int D)
{
    host_case("fir_filter_ccf", [D] { return blocks::fir_filter_ccf::make(lowpass(31, 0.4 / D), D); }, CSZ, CSZ, 1, (uint64_t)D, 100003);
}
TEST(HostRateTags, FirDecim1) { host_fir_case(1); }
TEST(HostRateTags, FirDecim2) { host_fir_case(2); }
TEST(HostRateTags, FirDecim4) { host_fir_case(4); }
TEST(HostRateTags, FirDecim8) { host_fir_case(8); }

// ---- 2: the other fixed-ratio decimators, offsets in items of each port ----------------------------
TEST(HostRateTags, XlatingFirDecim5)
{
    host_case("freq_xlating_fir_filter_ccf", [] { return blocks::freq_xlating_fir_filter_ccf::make(5, lowpass(31, 0.08), 0.1, 1.0); },
              CSZ, CSZ, 1, 5, 100003);
}
TEST(HostRateTags, XlatingFftFilterDecim4)
{
    host_case("freq_xlating_fft_filter_ccc",
              [] { return blocks::freq_xlating_fft_filter_ccc::make(4, complex_taps(lowpass(31, 0.1)), 0.1, 1.0); }, CSZ, CSZ, 1, 4,
              100003);
}
TEST(HostRateTags, PfbChannelizerM8)
{
    host_case("pfb_channelizer_ccf", [] { return blocks::pfb_channelizer_ccf::make(8, lowpass(64, 0.05)); }, CSZ, 8 * CSZ, 1, 8,
              100003);
}
TEST(HostRateTags, PsdN64K4)
{
    host_case("psd_vcf", [] { return blocks::psd_vcf::make(64, 4); }, 64 * CSZ, 64 * sizeof(float), 1, 4, 40001);
}

// ---- 3: 1:M, the tag lands on the first of its M outputs -------------------------------------------
TEST(HostRateTags, PfbSynthesizerM8)
{
    host_case("pfb_synthesizer_ccf", [] { return blocks::pfb_synthesizer_ccf::make(8, lowpass(64, 0.05)); }, 8 * CSZ, CSZ, 8, 1, 40001);
}

// ---- 4: I:D ------------------------------------------------------------------------------------------
TEST(HostRateTags, RationalResampler3over2)
{
    host_case("rational_resampler_ccf 3/2", [] { return blocks::rational_resampler_ccf::make(3, 2, lowpass(48, 0.15)); }, CSZ, CSZ, 3,
              2, 100003);
}
TEST(HostRateTags, RationalResampler2over3)
{
    host_case("rational_resampler_ccf 2/3", [] { return blocks::rational_resampler_ccf::make(2, 3, lowpass(48, 0.15)); }, CSZ, CSZ, 2,
              3, 100003);
}
// a ratio at which the rule in double arithmetic misplaces a tag: 45 * fl(7 / 5) rounds below 63
TEST(HostRateTags, RationalResampler7over5)
{
    EXPECT_TRUE(std::floor(45 * (7.0 / 5.0)) == 62.0);
    host_case("rational_resampler_ccf 7/5", [] { return blocks::rational_resampler_ccf::make(7, 5, lowpass(70, 0.06)); }, CSZ, CSZ, 7,
              5, 100003);
}

// ---- 5: any rate ---------------------------------------------------------------------------------------
TEST(HostRateTags, ArbResampler0p9) { host_arb_case(0.9); }
TEST(HostRateTags, ArbResampler1p37) { host_arb_case(1.37); }
// r = 1/64 fed five items at a time: most calls consume and produce nothing, and a tag consumed
// by such a call waits on the next item to be written
TEST(HostRateTags, ArbResamplerAdvancingCalls)
{
    const double rate = 1.0 / 64;
    const size_t n = 64 * 700 + 17;
    for (uint64_t when : { (uint64_t)997, (uint64_t)1 }) {
        auto fg = flowgraph::make();
        auto src = blocks::null_source::make(CSZ);
        auto head = blocks::head::make(CSZ, n);
        auto ann0 = A::make(when, CSZ, 1, 1, ALL);
        auto slow = trickle::make(5);
        auto blk = blocks::pfb_arb_resampler_ccf::make(rate, arb_taps(2048, 32, rate), 32);
        auto ann1 = A::make(1u << 30, CSZ, 1, 1, ALL);
        auto snk = blocks::null_sink::make(CSZ);
        fg->connect(src, 0, head, 0);
        fg->connect(head, 0, ann0, 0);
        fg->connect(ann0, 0, slow, 0);
        fg->connect(slow, 0, blk, 0);
        fg->connect(blk, 0, ann1, 0);
        fg->connect(ann1, 0, snk, 0);
        fg->set_scheduler(schedulers::scheduler_mt::make("mt", 4096));
        fg->validate();
        fg->run();
        std::printf("  %llu advancing calls\n", (unsigned long long)blk->advancing_calls());
        EXPECT_TRUE(blk->advancing_calls() > 0);
        check_arb(pairs_of(ann1), when, rate, n, snk->consumed(), label("pfb_arb_resampler_ccf 1/64", when, 4096));
    }
}

// ---- 6: policies on a D = 4 FIR --------------------------------------------------------------------------
static void host_policy_case(tag_propagation_policy_t pol, bool arrives)
{
    const size_t n = 100003;
    for (uint64_t when : { (uint64_t)997, (uint64_t)1 })
        for (unsigned buf : { 4096u, 1u << 20 }) {
            auto fir = blocks::fir_filter_ccf::make(lowpass(31, 0.1), 4);
            fir->set_tag_propagation_policy(pol);
            const pairs got = pairs_of(run_on_mt(fir, CSZ, CSZ, when, n, buf).sink);
            EXPECT_TRUE(same(got, arrives ? closed_form(when, n, 1, 4) : pairs{}, label("fir_filter_ccf D=4 policy", when, buf)));
        }
}
TEST(HostRateTags, PolicyDont) { host_policy_case(DONT, false); }
TEST(HostRateTags, PolicyOneToOne) { host_policy_case(ONE, true); }

TEST(HostRateTags, FanOutTwoReaders)
{
    const size_t n = 100003;
    for (uint64_t when : { (uint64_t)997, (uint64_t)1 })
        for (unsigned buf : { 4096u, 1u << 20 }) {
            auto fg = flowgraph::make();
            auto src = blocks::null_source::make(CSZ);
            auto head = blocks::head::make(CSZ, n);
            auto ann0 = A::make(when, CSZ, 1, 1, ALL);
            auto fir = blocks::fir_filter_ccf::make(lowpass(31, 0.1), 4);
            auto ann1 = A::make(1u << 30, CSZ, 1, 1, ALL);
            auto ann2 = A::make(1u << 30, CSZ, 1, 1, ALL);
            auto snk1 = blocks::null_sink::make(CSZ);
            auto snk2 = blocks::null_sink::make(CSZ);
            fg->connect(src, 0, head, 0);
            fg->connect(head, 0, ann0, 0);
            fg->connect(ann0, 0, fir, 0);
            fg->connect(fir, 0, ann1, 0);
            fg->connect(fir, 0, ann2, 0);
            fg->connect(ann1, 0, snk1, 0);
            fg->connect(ann2, 0, snk2, 0);
            fg->set_scheduler(schedulers::scheduler_mt::make("mt", buf));
            fg->validate();
            fg->run();
            const pairs want = closed_form(when, n, 1, 4);
            EXPECT_TRUE(same(pairs_of(ann1), want, label("first reader", when, buf)));
            EXPECT_TRUE(same(pairs_of(ann2), want, label("second reader", when, buf)));
        }
}

// add_cc (rate 1) under ALL_TO_ALL with a tagged stream on each input: the annotator numbers its
// two outputs' tags 2k and 2k + 1 at offset k when, and the sink sees both (per call one input's
// tags, then the other's: compared sorted)
TEST(HostRateTags, AddTwoTaggedInputs)
{
    const size_t n = 100003;
    for (uint64_t when : { (uint64_t)997, (uint64_t)1 })
        for (unsigned buf : { 4096u, 1u << 20 }) {
            auto fg = flowgraph::make();
            auto src = blocks::null_source::make(CSZ);
            auto head = blocks::head::make(CSZ, n);
            auto ann0 = A::make(when, CSZ, 1, 2, ALL);
            auto add = blocks::add_cc::make(2);
            auto ann1 = A::make(1u << 30, CSZ, 1, 1, ALL);
            auto snk = blocks::null_sink::make(CSZ);
            fg->connect(src, 0, head, 0);
            fg->connect(head, 0, ann0, 0);
            fg->connect(ann0, 0, add, 0);
            fg->connect(ann0, 1, add, 1);
            fg->connect(add, 0, ann1, 0);
            fg->connect(ann1, 0, snk, 0);
            fg->set_scheduler(schedulers::scheduler_mt::make("mt", buf));
            fg->validate();
            fg->run();
            pairs got = pairs_of(ann1), want;
            std::sort(got.begin(), got.end());
            for (uint64_t t = 0; t < n; t += when) {
                want.emplace_back((int64_t)(2 * (t / when)), t);
                want.emplace_back((int64_t)(2 * (t / when) + 1), t);
            }
            EXPECT_TRUE(same(got, want, label("add_cc", when, buf)));
        }
}

// ---- 7: the D = 4 FIR alone in a domain of its own, as SchedulerMTTags.AcrossDomains ---------------
TEST(HostRateTags, AcrossDomains)
{
    const size_t n = 100003;
    for (uint64_t when : { (uint64_t)997, (uint64_t)1 })
        for (unsigned buf : { 4096u, 1u << 20 }) {
            auto fir = blocks::fir_filter_ccf::make(lowpass(31, 0.1), 4);
            auto fg = flowgraph::make();
            auto src = blocks::null_source::make(CSZ);
            auto head = blocks::head::make(CSZ, n);
            auto ann0 = A::make(when, CSZ, 1, 1, ALL);
            auto ann1 = A::make(1u << 30, CSZ, 1, 1, ALL);
            auto snk = blocks::null_sink::make(CSZ);
            fg->connect(src, 0, head, 0);
            fg->connect(head, 0, ann0, 0);
            fg->connect(ann0, 0, fir, 0);
            fg->connect(fir, 0, ann1, 0);
            fg->connect(ann1, 0, snk, 0);
            auto a = schedulers::scheduler_mt::make("a", buf);
            auto b = schedulers::scheduler_mt::make("b", buf);
            auto c = schedulers::scheduler_mt::make("c", buf);
            fg->add_scheduler(a);
            fg->add_scheduler(b);
            fg->add_scheduler(c);
            auto da = domain_adapter_direct_conf::make(buffer_preference_t::DOWNSTREAM);
            domain_conf_vec dc{ domain_conf(a, { src, head, ann0 }, da), domain_conf(b, { fir }, da), domain_conf(c, { ann1, snk }, da) };
            fg->partition(dc);
            fg->run();
            EXPECT_TRUE(same(pairs_of(ann1), closed_form(when, n, 1, 4), label("fir_filter_ccf D=4 across domains", when, buf)));
        }
}

// ---- 8: restart. The first run leaves 3 of its 100003 items unread; they are dropped, and the second
// run's tags count from the counters it started with, (100003, 25000): the tag at 100697 lands on
// 25000 + floor(694 / 4) = 25173, where floor(100697 / 4) = 25174 would put it one late.
TEST(HostRateTags, Restart)
{
    const size_t n = 100003;
    for (unsigned buf : { 4096u, 1u << 20 }) {
        auto fg = flowgraph::make();
        auto src = blocks::vector_source_c::make(std::vector<gr_complex>(n));
        auto ann0 = A::make(997, CSZ, 1, 1, ALL);
        auto fir = blocks::fir_filter_ccf::make(lowpass(31, 0.1), 4);
        auto ann1 = A::make(1u << 30, CSZ, 1, 1, ALL);
        auto snk = blocks::null_sink::make(CSZ);
        fg->connect(src, 0, ann0, 0);
        fg->connect(ann0, 0, fir, 0);
        fg->connect(fir, 0, ann1, 0);
        fg->connect(ann1, 0, snk, 0);
        fg->set_scheduler(schedulers::scheduler_mt::make("mt", buf));
        fg->validate();
        fg->run();
        const pairs first = pairs_of(ann1);
        EXPECT_TRUE(same(first, closed_form(997, n, 1, 4), label("first run", 997, buf)));
        fg->run();
        const pairs second = pairs_of(ann1, first.size());
        const pairs want = closed_form(997, n, 1, 4, n, n / 4);
        EXPECT_TRUE(want.front() == std::make_pair((int64_t)101, (uint64_t)25173));
        EXPECT_TRUE(same(second, want, label("second run", 997, buf)));
    }
}

// ---- 9: every rate-changing gr::hip block between an H2D and a D2H edge ----------------------------
TEST(DeviceRateTags, FirDecim4)
{
    device_case("hip::fir_filter_ccf D=4", [] { return hip::fir_filter_ccf::make(lowpass(127, 0.1), 4); }, CSZ, CSZ, 1, 4, 40003);
}
TEST(DeviceRateTags, FirDecim16Pfft)
{
    hip::fir_filter_ccf::sptr last;
    device_case("hip::fir_filter_ccf D=16", [&last] { return last = hip::fir_filter_ccf::make(lowpass(127, 0.03), 16); }, CSZ, CSZ, 1, 16,
                40003);
    EXPECT_TRUE(last->kernel() == "k_fir_pfft2<16>"); // the single-stage polyphase-FFT form
}
TEST(DeviceRateTags, XlatingFirDecim5)
{
    device_case("hip::freq_xlating_fir_filter_ccf", [] { return hip::freq_xlating_fir_filter_ccf::make(5, lowpass(63, 0.08), 0.1, 1.0); },
                CSZ, CSZ, 1, 5, 40003);
}
TEST(DeviceRateTags, XlatingFftFilterDecim4)
{
    device_case("hip::freq_xlating_fft_filter_ccc",
                [] { return hip::freq_xlating_fft_filter_ccc::make(4, complex_taps(lowpass(127, 0.1)), 0.1, 1.0); }, CSZ, CSZ, 1, 4, 40003);
}
TEST(DeviceRateTags, PfbChannelizerM8)
{
    device_case("hip::pfb_channelizer_ccf", [] { return hip::pfb_channelizer_ccf::make(8, lowpass(64, 0.05)); }, CSZ, 8 * CSZ, 1, 8,
                40003);
}
TEST(DeviceRateTags, PfbSynthesizerM8)
{
    device_case("hip::pfb_synthesizer_ccf", [] { return hip::pfb_synthesizer_ccf::make(8, lowpass(64, 0.05)); }, 8 * CSZ, CSZ, 8, 1,
                10001);
}
TEST(DeviceRateTags, RationalResampler3over2)
{
    device_case("hip::rational_resampler_ccf 3/2", [] { return hip::rational_resampler_ccf::make(3, 2, lowpass(48, 0.15)); }, CSZ, CSZ,
                3, 2, 40003);
}
TEST(DeviceRateTags, PsdN64K4)
{
    device_case("hip::psd_vcf", [] { return hip::psd_vcf::make(64, 4); }, 64 * CSZ, 64 * sizeof(float), 1, 4, 10001);
}
TEST(DeviceRateTags, FftN64)
{
    device_case("hip::fft_vcc", [] { return hip::fft_vcc::make(64); }, 64 * CSZ, 64 * CSZ, 1, 1, 10001);
}
TEST(DeviceRateTags, FftFilter)
{
    device_case("hip::fft_filter_ccc", [] { return hip::fft_filter_ccc::make(complex_taps(lowpass(127, 0.1))); }, CSZ, CSZ, 1, 1, 40003);
}
TEST(DeviceRateTags, ArbResampler0p9)
{
    const double rate = 0.9;
    const size_t n = 40003;
    for (uint64_t when : { (uint64_t)997, (uint64_t)1 }) {
        auto g = run_on_mt(hip::pfb_arb_resampler_ccf::make(rate, arb_taps(256, 32, rate), 32), CSZ, CSZ, when, n, 32768, true);
        check_arb(pairs_of(g.sink), when, rate, n, g.snk->consumed(), label("hip::pfb_arb_resampler_ccf", when, 32768));
    }
}

// ---- 10: 4 x hip::fir_filter_ccf(127 taps, D = 2) in a scheduler_hip domain, fused into one
// fir_filter_cascade_ccf and staged. floor(t / 16) equals four nested floors by 2, so the fused
// block propagates as one decimating block and both lists are the same closed form.
static pairs cascade_tags(bool fused, uint64_t when, size_t n)
{
    const auto h = lowpass(127, 0.225);
    auto fg = flowgraph::make();
    auto src = blocks::null_source::make(CSZ);
    auto head = blocks::head::make(CSZ, n);
    auto ann0 = A::make(when, CSZ, 1, 1, ALL);
    std::vector<hip::fir_filter_ccf::sptr> st;
    for (int i = 0; i < 4; ++i) st.push_back(hip::fir_filter_ccf::make(h, 2));
    auto ann1 = A::make(1u << 30, CSZ, 1, 1, ALL);
    auto snk = blocks::null_sink::make(CSZ);
    fg->connect(src, 0, head, 0);
    fg->connect(head, 0, ann0, 0);
    fg->connect(ann0, 0, st[0], 0)->set_custom_buffer(HIP_BUFFER_ARGS_H2D);
    for (int i = 1; i < 4; ++i) fg->connect(st[i - 1], 0, st[i], 0);
    fg->connect(st[3], 0, ann1, 0)->set_custom_buffer(HIP_BUFFER_ARGS_D2H);
    fg->connect(ann1, 0, snk, 0);
    auto cpu = schedulers::scheduler_mt::make("cpu", 32768);
    auto gpu = schedulers::scheduler_hip::make("gpu", 0, 1u << 16);
    gpu->set_fir_fusion(fused);
    fg->add_scheduler(cpu);
    fg->add_scheduler(gpu);
    auto da = domain_adapter_direct_conf::make(buffer_preference_t::DOWNSTREAM);
    domain_conf_vec dc{ domain_conf(cpu, { src, head, ann0, ann1, snk }, da), domain_conf(gpu, { st[0], st[1], st[2], st[3] }, da) };
    fg->partition(dc);
    const auto& plan = gpu->fusion_plan().fused;
    if (fused)
        EXPECT_TRUE(plan.size() == 1u && std::dynamic_pointer_cast<hip::fir_filter_cascade_ccf>(plan[0]) != nullptr);
    else
        EXPECT_TRUE(plan.empty());
    fg->run();
    return pairs_of(ann1);
}
TEST(DeviceRateTags, FusedCascade)
{
    const size_t n = 40003;
    for (uint64_t when : { (uint64_t)997, (uint64_t)1 }) {
        const pairs want = closed_form(when, n, 1, 16);
        const pairs fused = cascade_tags(true, when, n), staged = cascade_tags(false, when, n);
        EXPECT_TRUE(same(fused, want, label("fused cascade", when, 1u << 16)));
        EXPECT_TRUE(same(staged, want, label("staged cascade", when, 1u << 16)));
        EXPECT_TRUE(fused == staged);
    }
}
