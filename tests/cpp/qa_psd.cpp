// psd_vcf through the runtime.
//   PsdCpu.*  the CPU block (it defines the semantics) on scheduler_mt with small buffers, so the
//             stream passes through many work() calls, against an in-test double computation (an
//             O(N^2) DFT from the definition at N = 16 and 64, a radix-2 FFT at 1024), input counts
//             that are no multiple of navg, dB, and what the constructors of both blocks refuse.
//   PsdHip.*  the GPU block in a scheduler_hip domain fed from / drained into a scheduler_mt domain
//             over H2D / D2H edges, against the in-test double computation within the bound below
//             and against the CPU block, at (N, K) = (64, 5), (1024, 16), (4096, 100); work() calls
//             whose input counts are no multiples of K; a restart (bit-identical: a vector's value
//             does not depend on how the stream is cut); dB; the block's kernel timing.
// Bound (tests/test_gpu_psd.py, include/nsh_hip.h): with X_f the double transform of frame f,
// d_f = 1e-5 max_k |X_f[k]|, g = (K + 2) 2^-24,
//   |out[k] - P[k]| <= B[k] = scale [sum_f (2 |X_f[k]| d_f + d_f^2) + g sum_f |X_f[k]|^2]
// dB: bins with B/P <= 0.1 by |d| <= (10 / ln 10) (B/P) / (1 - B/P) + 8 2^-24 max(|dB|, 1), the
// others in the linear domain through 10^(out/10) with bound 2 B.
#include "qa.hpp"

#include <cmath>
#include <complex>
#include <stdexcept>
#include <gnuradio/blocklib/blocks/psd.hpp>
#include <gnuradio/blocklib/blocks/vector_sink.hpp>
#include <gnuradio/blocklib/blocks/vector_source.hpp>
#include <gnuradio/blocklib/hip/psd.hpp>
#include <gnuradio/domain_adapter_direct.hpp>
#include <gnuradio/flowgraph.hpp>
#include <gnuradio/hip_buffer.hpp>
#include <gnuradio/schedulers/hip/scheduler_hip.hpp>
#include <gnuradio/schedulers/mt/scheduler_mt.hpp>

#include "nsh_hip.h"

using namespace gr;

#include "qa_ref.hpp"

namespace {

using cd = std::complex<double>;

std::vector<float> hann(size_t N)
{
    std::vector<float> w(N);
    for (size_t n = 0; n < N; ++n) w[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)n / (double)N));
    return w;
}

// the windowed frame (fp32 products) transformed in double: from the definition, or radix-2
std::vector<cd> transform(const gr_complex* x, size_t N, const std::vector<float>& w, bool direct)
{
    std::vector<cd> a(N), X(N);
    for (size_t n = 0; n < N; ++n) {
        const float wv = w.empty() ? 1.f : w[n];
        a[n] = { (double)(x[n].real() * wv), (double)(x[n].imag() * wv) };
    }
    if (direct) {
        for (size_t k = 0; k < N; ++k) {
            cd s = 0;
            for (size_t n = 0; n < N; ++n) s += a[n] * std::polar(1.0, -2.0 * M_PI * (double)((k * n) % N) / (double)N);
            X[k] = s;
        }
        return X;
    }
    size_t bits = 0;
    while (((size_t)1 << bits) < N) ++bits;
    for (size_t n = 0; n < N; ++n) {
        size_t rev = 0;
        for (size_t b = 0; b < bits; ++b) rev |= ((n >> b) & 1) << (bits - 1 - b);
        X[rev] = a[n];
    }
    for (size_t len = 2; len <= N; len <<= 1)
        for (size_t i = 0; i < N; i += len)
            for (size_t k = 0; k < len / 2; ++k) {
                const cd u = X[i + k], v = X[i + k + len / 2] * std::polar(1.0, -2.0 * M_PI * (double)k / (double)len);
                X[i + k] = u + v;
                X[i + k + len / 2] = u - v;
            }
    return X;
}

struct psd_ref {
    std::vector<double> p, b; // P_j[k] (shifted, linear) and the bound B_j[k], nvec * N each
};
psd_ref reference(const std::vector<gr_complex>& x, size_t N, size_t K, const std::vector<float>& w, bool shift, double scale,
                  bool direct)
{
    const size_t nvec = x.size() / (N * K);
    psd_ref r;
    r.p.assign(nvec * N, 0.0);
    r.b.assign(nvec * N, 0.0);
    const double g = (double)(K + 2) * std::ldexp(1.0, -24);
    for (size_t j = 0; j < nvec; ++j) {
        std::vector<double> sum(N, 0.0), lin(N, 0.0);
        for (size_t f = 0; f < K; ++f) {
            const auto X = transform(x.data() + (j * K + f) * N, N, w, direct);
            double mx = 0;
            for (auto& v : X) mx = std::max(mx, std::abs(v));
            const double d = 1e-5 * mx;
            for (size_t k = 0; k < N; ++k) {
                sum[k] += std::norm(X[k]);
                lin[k] += 2 * std::abs(X[k]) * d + d * d;
            }
        }
        for (size_t k = 0; k < N; ++k) {
            const size_t src = shift ? k ^ (N / 2) : k;
            r.p[j * N + k] = scale * sum[src];
            r.b[j * N + k] = scale * (lin[src] + g * sum[src]);
        }
    }
    return r;
}

// y against the reference: linear within B (plus tol_rel |P|: the rounding of a float computed in
// double), or dB by the rule above; prints and returns the worst err / bound
double worst_ratio(const std::vector<float>& y, const psd_ref& r, bool db, double tol_rel = 0)
{
    if (y.size() != r.p.size()) {
        std::fprintf(stderr, "  size %zu != %zu\n", y.size(), r.p.size());
        return INFINITY;
    }
    double worst = 0;
    for (size_t i = 0; i < y.size(); ++i) {
        const double P = r.p[i], B = r.b[i] + tol_rel * P;
        double ratio;
        if (!db)
            ratio = std::abs((double)y[i] - P) / B;
        else if (B / P <= 0.1) {
            const double ref = 10.0 * std::log10(P), q = B / P;
            ratio = std::abs((double)y[i] - ref) / (10.0 / std::log(10.0) * q / (1 - q) + 8 * std::ldexp(1.0, -24) * std::max(std::abs(ref), 1.0));
        } else
            ratio = std::abs(std::pow(10.0, (double)y[i] / 10.0) - P) / (2 * B);
        if (!(ratio <= worst)) worst = ratio; // a NaN sticks
    }
    return worst;
}

// vector_source(vlen N) -> blk -> vector_sink_f(vlen N) on one scheduler_mt with small buffers
std::vector<float> run_cpu(const block_sptr& blk, const std::vector<gr_complex>& x, size_t N, size_t K)
{
    auto src = blocks::vector_source_c::make(x, false, (unsigned)N);
    auto snk = blocks::vector_sink_f::make(N, x.size() / N / K + 1);
    auto fg = flowgraph::make();
    fg->connect(src, 0, blk, 0);
    fg->connect(blk, 0, snk, 0);
    fg->set_scheduler(schedulers::scheduler_mt::make("mt", (unsigned)std::max<size_t>(8192, 4 * N * sizeof(gr_complex))));
    fg->validate();
    fg->run();
    return snk->data();
}

struct hip_run {
    flowgraph_sptr fg;
    blocks::vector_sink_f::sptr snk;
    std::shared_ptr<schedulers::scheduler_hip> gpu;
};
// vector_source(vlen N) -[H2D]-> blk -[D2H]-> vector_sink_f(vlen N): a scheduler_mt domain and a
// scheduler_hip domain, 64 KiB rings (8 items where those are larger; the runtime sizes the edge
// into a decimator for at least 2 K items)
hip_run make_hip(const block_sptr& blk, const std::vector<gr_complex>& x, size_t N, size_t K)
{
    hip_run r;
    auto src = blocks::vector_source_c::make(x, false, (unsigned)N);
    r.snk = blocks::vector_sink_f::make(N, x.size() / N / K + 1);
    r.fg = flowgraph::make();
    r.fg->connect(src, 0, blk, 0)->set_custom_buffer(HIP_BUFFER_ARGS_H2D);
    r.fg->connect(blk, 0, r.snk, 0)->set_custom_buffer(HIP_BUFFER_ARGS_D2H);
    const unsigned ring = (unsigned)std::max<size_t>(1u << 16, 8 * N * sizeof(gr_complex));
    auto cpu = schedulers::scheduler_mt::make("cpu", ring);
    r.gpu = schedulers::scheduler_hip::make("gpu", 0, ring);
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

// noise with a tone at a bin centre and one off it
std::vector<gr_complex> signal(size_t n, size_t N, uint64_t seed)
{
    auto x = synth(n, 0, seed);
    for (size_t i = 0; i < n; ++i) {
        const double a = 2.0 * M_PI * (double)(N / 8) * (double)i / (double)N, b = 2.0 * M_PI * ((double)(N / 3) + 0.37) * (double)i / (double)N;
        x[i] = gr_complex(0.01f * x[i].real() + (float)(std::cos(a) + 0.5 * std::cos(b)), 0.01f * x[i].imag() + (float)(std::sin(a) + 0.5 * std::sin(b)));
    }
    return x;
}

} // namespace

// ---- CPU block ---------------------------------------------------------------------------------
// extra: input vectors beyond nvec whole groups, which the block must leave unconsumed
static void cpu_case(size_t N, size_t K, size_t nvec, size_t extra, bool window, bool shift, float scale, bool db, bool direct)
{
    const auto x = signal((nvec * K + extra) * N, N, 1000 + N + K);
    const auto w = window ? hann(N) : std::vector<float>{};
    auto blk = blocks::psd_vcf::make(N, K, w, shift, scale, db);
    EXPECT_EQ(blk->fft_size(), N);
    EXPECT_EQ(blk->navg(), K);
    EXPECT_TRUE(blk->shift() == shift && blk->db() == db && blk->window() == w);
    const float used = scale == 0.f ? 1.f / (float)K : scale;
    EXPECT_TRUE(blk->scale() == used);
    const auto y = run_cpu(blk, x, N, K);
    ASSERT_TRUE(y.size() == nvec * N);
    auto ref = reference(std::vector<gr_complex>(x.begin(), x.begin() + nvec * K * N), N, K, w, shift, used, direct);
    // double throughout, rounded once: half an ulp of the float, and 1e-12 of the vector's largest
    // bin for the difference between two double transforms
    double pmax = 0;
    for (double p : ref.p) pmax = std::max(pmax, p);
    for (auto& b : ref.b) b = 0;
    for (size_t i = 0; i < ref.p.size(); ++i) ref.b[i] = std::ldexp(1.0, -24) * ref.p[i] + 1e-12 * pmax;
    const double worst = worst_ratio(y, ref, db);
    std::printf("  cpu N=%zu K=%zu db=%d: worst err / bound %.3g\n", N, K, (int)db, worst);
    EXPECT_TRUE(worst <= 1.0);
}
TEST(PsdCpu, N16AgainstDft)
{
    cpu_case(16, 1, 40, 0, false, false, 1.f, false, true);
    cpu_case(16, 7, 9, 3, true, true, 0.f, false, true);
}
TEST(PsdCpu, N64AgainstDft)
{
    cpu_case(64, 5, 11, 4, true, false, 0.f, false, true);
    cpu_case(64, 3, 6, 1, false, true, 0.125f, false, true);
}
TEST(PsdCpu, N1024AgainstFft) { cpu_case(1024, 16, 3, 5, true, true, 0.f, false, false); }
TEST(PsdCpu, Decibels)
{
    // the dB rule with the rounding bound: |d| <= (10 / ln 10) q / (1 - q) + 8 2^-24 max(|dB|, 1)
    cpu_case(64, 5, 7, 0, true, true, 0.f, true, true);
}
TEST(PsdCpu, RefusesBadArguments)
{
    const float nan = std::nanf(""), inf = INFINITY;
    for (size_t bad : { (size_t)0, (size_t)8, (size_t)24, (size_t)1000, (size_t)16384 }) {
        EXPECT_TRUE(refused([bad] { blocks::psd_vcf::make(bad, 4); }));
        EXPECT_TRUE(refused([bad] { hip::psd_vcf::make(bad, 4); }));
    }
    for (size_t bad : { (size_t)0, (size_t)65537, (size_t)1 << 20 }) {
        EXPECT_TRUE(refused([bad] { blocks::psd_vcf::make(64, bad); }));
        EXPECT_TRUE(refused([bad] { hip::psd_vcf::make(64, bad); }));
    }
    EXPECT_TRUE(refused([] { blocks::psd_vcf::make(64, 4, std::vector<float>(63, 1.f)); }));
    EXPECT_TRUE(refused([] { hip::psd_vcf::make(64, 4, std::vector<float>(128, 1.f)); }));
    std::vector<float> w(64, 1.f);
    w[17] = nan;
    EXPECT_TRUE(refused([&] { blocks::psd_vcf::make(64, 4, w); }));
    EXPECT_TRUE(refused([&] { hip::psd_vcf::make(64, 4, w); }));
    for (float bad : { nan, inf, -inf, -1.f }) {
        EXPECT_TRUE(refused([bad] { blocks::psd_vcf::make(64, 4, {}, false, bad); }));
        EXPECT_TRUE(refused([bad] { hip::psd_vcf::make(64, 4, {}, false, bad); }));
    }
    EXPECT_FALSE(refused([] { blocks::psd_vcf::make(16, 1); }));
    EXPECT_FALSE(refused([] { blocks::psd_vcf::make(8192, 65536, hann(8192), true, 2.f, true); }));
    EXPECT_FALSE(refused([] { hip::psd_vcf::make(16, 1); }));
    auto h = hip::psd_vcf::make(8192, 65536, hann(8192), true, 0.f, true);
    EXPECT_EQ(h->fft_size(), (size_t)8192);
    EXPECT_EQ(h->navg(), (size_t)65536);
    EXPECT_EQ(h->decimation(), 65536u);
    EXPECT_TRUE(h->shift() && h->db() && h->window() == hann(8192) && h->scale() == 1.f / 65536.f);
    EXPECT_TRUE(h->kernel().empty()); // no plan before start()
}

// ---- GPU block ---------------------------------------------------------------------------------
static void hip_case(size_t N, size_t K, size_t nvec, size_t extra, bool shift, bool db)
{
    const auto x = signal((nvec * K + extra) * N, N, 2000 + N + K);
    const auto w = hann(N);
    const float scale = 1.f / (float)K;
    const auto ref = reference(std::vector<gr_complex>(x.begin(), x.begin() + nvec * K * N), N, K, w, shift, scale, false);
    const auto cpu = run_cpu(blocks::psd_vcf::make(N, K, w, shift, 0.f, db), x, N, K);
    auto blk = hip::psd_vcf::make(N, K, w, shift, 0.f, db);
    auto r = make_hip(blk, x, N, K);
    r.fg->run();
    const auto y = r.snk->data();
    ASSERT_TRUE(y.size() == nvec * N);
    ASSERT_TRUE(cpu.size() == nvec * N);
    const double worst = worst_ratio(y, ref, db);
    // against the CPU block: the same rule around the CPU block's spectrum (10^(dB / 10) in dB mode),
    // plus the rounding of the CPU block's float: 2^-24 of the value, in dB 2^-24 |dB|, which is
    // (ln 10 / 10) 2^-24 |dB| of the spectrum
    psd_ref vs_cpu = ref;
    double cpu_round = std::ldexp(1.0, -24);
    if (db) {
        double dmax = 1;
        for (float v : cpu) dmax = std::max(dmax, (double)std::abs(v));
        cpu_round *= std::log(10.0) / 10.0 * dmax;
    }
    for (size_t i = 0; i < cpu.size(); ++i) vs_cpu.p[i] = db ? std::pow(10.0, (double)cpu[i] / 10.0) : (double)cpu[i];
    const double worst_cpu = worst_ratio(y, vs_cpu, db, cpu_round);
    std::printf("  hip N=%zu K=%zu db=%d: %s, %llu launches, worst err / bound %.3g (vs the CPU block %.3g)\n", N, K, (int)db,
                blk->kernel().c_str(), (unsigned long long)blk->launches(), worst, worst_cpu);
    EXPECT_TRUE(worst <= 1.0);
    EXPECT_TRUE(worst_cpu <= 1.0);
    EXPECT_TRUE(blk->launches() > 1); // the stream passed through several work() calls
    r.fg->run();                      // the plan survives a restart; the cut of the stream does not matter
    EXPECT_TRUE(r.snk->data() == y);
}
TEST(PsdHip, N64K5) { hip_case(64, 5, 2001, 3, false, false); }
TEST(PsdHip, N1024K16Shift) { hip_case(1024, 16, 41, 7, true, false); }
TEST(PsdHip, N4096K100) { hip_case(4096, 100, 5, 17, false, false); }
TEST(PsdHip, Decibels)
{
    hip_case(64, 5, 501, 0, true, true);
    hip_case(4096, 100, 5, 0, false, true);
}

// the block's own timing arms a pair per work(), taken by the call's one or two launches
TEST(PsdHip, KernelTiming)
{
    for (size_t K : { (size_t)5, (size_t)40 }) { // one segment; several, through the plan's scratch
        const size_t N = 1024, nvec = 60;
        const auto x = signal(nvec * K * N, N, 9);
        auto blk = hip::psd_vcf::make(N, K);
        auto r = make_hip(blk, x, N, K);
        blk->enable_timing(true);
        r.fg->run();
        EXPECT_EQ(r.snk->data().size(), nvec * N);
        EXPECT_EQ(blk->timed_vectors(), (uint64_t)nvec);
        EXPECT_TRUE(blk->kernel_ms() > 0); // throws if an armed pair went unrecorded
    }
}
