// libnsh_hip.so: fft_filter_ccc, a FIR filter with complex taps by overlap-save in one launch.
//
//   y[n] = sum_{k<L} h[k] x[n-k],   x, h complex fp32, 1 <= L <= 4096, decimation 1
//
// Frames of N in {1024, 2048, 4096, 8192} samples, L <= N/2, H = L-1, V = N-H valid outputs each:
// frame f owns out[fV, (f+1)V) and reads the window x[fV-H, fV-H+N) (history or zeros below 0, zeros
// at or past n). A team of geom<N>::TT lanes (nsh_fft_team.hpp) holds one frame, 16 samples a lane:
//
//   window -> fft_team<N, false> -> times Hs -> out_idx to in_idx order through the team's image
//          -> fft_team<N, true> -> store of the samples at in-frame index >= H
//
// Hs[k] = (1/N) sum_{n<L} h[n] e^{-2 pi i kn/N}, computed in double on the host and rounded once; the
// table lies in the order the lanes meet it after the forward transform (entry m TT + t is
// Hs[geom::out_idx(t, m)]), so a wave reads it as whole lines. A lane meets the same 16 entries in
// every frame: N <= 4096 keeps them in registers for the whole kernel, N = 8192 (512 lanes, 256
// VGPRs each) reads them from L2 after every forward transform.
//
// Windows start at any 8-byte aligned sample and overlap, so a frame gets a buffer resource of its
// own: base in + (fV-H), length what is left of the stream, at most N. What lies past the end reads
// zeros without an address being formed for it, and the loop issues the same loads for every frame:
// the next frame's stay in flight across this frame's arithmetic. Only frame 0 of a call has
// positions below 0 (V - H >= 2); the team that owns it loads it before the loop, history and input
// through one resource each. Stores go through a resource over the frame's V outputs, clipped at
// out + n; the lanes below H get an offset no resource reaches.
#include "nsh_fft_ols.hpp"
#include "nsh_stream_tile.hpp"

#include <cmath>
#include <memory>
#include <string>
#include <vector>

namespace {

using nsh::cf;
using nsh::cmulw;
using nsh::fft::fft_team;
using nsh::fft::geom;
using nsh::fft::pad;
using nsh::fft::team_sync;
using nsh::ols::buf_load_cf;
using nsh::ols::default_cap;
using nsh::ols::default_fft_size;
using nsh::ols::kNowhere;
using nsh::ols::span_rsrc;
using nsh::ols::spectrum_of;

template <int N>
constexpr bool hs_in_regs = geom<N>::NT <= 256;

template <int N>
__global__ __launch_bounds__(geom<N>::NT) void k_fft_filter(const float2* __restrict__ in, const float2* __restrict__ hist_in,
                                                            float2* __restrict__ hist_out, float2* __restrict__ out, int64_t n,
                                                            int L, const float2* __restrict__ tw_g,
                                                            const float2* __restrict__ hs_g)
{
    using G = geom<N>;
    static_assert(G::F == 1, "one frame per team");
    constexpr bool HREG = hs_in_regs<N>;
    __shared__ cf tw[G::TWN];
    __shared__ cf img_all[G::TEAMS * G::IMG];
    nsh::fft::stage_table(tw, tw_g, G::TWN, threadIdx.x, G::NT);
    __syncthreads();
    const int t = threadIdx.x & (G::TT - 1), team = threadIdx.x / G::TT;
    cf* img = img_all + team * G::IMG;
    const int H = L - 1, V = N - H;
    const int64_t nframes = (n + V - 1) / V, ngroups = (nframes + G::TILE - 1) / G::TILE;

    // window of frame f >= 1
    const auto load_window = [&](cf(&v)[16], int64_t f) {
        const int64_t w0 = f * V - H;
        int64_t items = n - w0;
        items = items < 0 ? 0 : (items > N ? N : items);
        const __amdgpu_buffer_rsrc_t r = span_rsrc(in + (items > 0 ? w0 : 0), items);
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = buf_load_cf(r, G::in_idx(t, m) * 8);
    };
    // window of frame 0: H samples of history (zeros without one), then the input
    const auto load_first = [&](cf(&v)[16]) {
        const __amdgpu_buffer_rsrc_t rh = span_rsrc(hist_in, hist_in ? H : 0);
        const __amdgpu_buffer_rsrc_t ri = span_rsrc(in, n < V ? n : V);
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const int p = G::in_idx(t, m);
            const cf a = buf_load_cf(rh, p < H ? p * 8 : kNowhere);
            const cf b = buf_load_cf(ri, p >= H ? (p - H) * 8 : kNowhere);
            v[m] = p < H ? a : b;
        }
    };

    int64_t g = blockIdx.x;
    if (g >= ngroups) return;
    cf hs[16];
    if constexpr (HREG) {
#pragma unroll
        for (int m = 0; m < 16; ++m) hs[m] = cf{ hs_g[m * G::TT + t].x, hs_g[m * G::TT + t].y };
    }
    // every team of the workgroup walks the same number of steps (workgroup barriers inside): a team
    // past the last frame loads zeros and its stores are dropped
    cf v[16], nx[16];
    if (g * G::TEAMS + team == 0)
        load_first(v);
    else
        load_window(v, g * G::TEAMS + team);
    for (; g < ngroups; g += gridDim.x) {
        const int64_t f = g * G::TEAMS + team;
        load_window(nx, f + (int64_t)gridDim.x * G::TEAMS);
        fft_team<N, false>(v, img, tw, t);
        if constexpr (!HREG) {
#pragma unroll
            for (int m = 0; m < 16; ++m) hs[m] = cf{ hs_g[m * G::TT + t].x, hs_g[m * G::TT + t].y };
        }
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = cmulw(v[m], hs[m]);
        // the spectrum lies as the forward transform left it; the inverse takes in_idx order
#pragma unroll
        for (int m = 0; m < 16; ++m) img[pad(G::out_idx(t, m))] = v[m];
        team_sync<G::WG>();
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = img[pad(G::in_idx(t, r))];
        team_sync<G::WG>();
        fft_team<N, true>(v, img, tw, t);
        {
            const int64_t o0 = f * V;
            int64_t items = n - o0;
            items = items < 0 ? 0 : (items > V ? V : items);
            const __amdgpu_buffer_rsrc_t r = span_rsrc(out + (items > 0 ? o0 : 0), items);
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const int i = G::out_idx(t, m);
                nsh::buf_store_f2(r, i >= H ? (i - H) * 8 : kNowhere, v[m]);
            }
        }
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = nx[m];
    }
    if (blockIdx.x == 0) nsh::store_history<G::NT>(in, hist_in, hist_out, n, L, threadIdx.x);
}

struct filter_plan {
    int dev = 0, n = 0, L = 0, tile = 0, cap = 0, cap_default = 0;
    float2* tw = nullptr;
    float2* hs = nullptr;
    std::string kernel;
    void (*launch)(const filter_plan*, const float2*, const float2*, float2*, float2*, int64_t, unsigned, hipStream_t) = nullptr;
    ~filter_plan()
    {
        nsh::dev_free(tw);
        nsh::dev_free(hs);
    }
};

template <int N>
void launch_filter(const filter_plan* p, const float2* in, const float2* hist_in, float2* hist_out, float2* out, int64_t n,
                   unsigned grid, hipStream_t s)
{
    nsh::launch((k_fft_filter<N>), dim3(grid), dim3(geom<N>::NT), 0, s, in, hist_in, hist_out, out, n, p->L,
                (const float2*)p->tw, (const float2*)p->hs);
}

// Hs in the lanes' order: entry m TT + t = Hs[out_idx(t, m)]
template <int N>
void setup(filter_plan* p, const std::vector<float2>& spectrum, std::vector<float2>& ordered)
{
    using G = geom<N>;
    p->tile = G::TILE;
    p->launch = launch_filter<N>;
    ordered.resize(N);
    for (int m = 0; m < 16; ++m)
        for (int t = 0; t < G::TT; ++t) ordered[m * G::TT + t] = spectrum[G::out_idx(t, m)];
}

} // namespace

extern "C" {

int nsh_fft_filter_plan_create(int dev, const float* taps_host, int ntaps, int fft_size, void** plan)
{
    if (!taps_host || !plan) return nsh::fail_msg("nsh_fft_filter_plan_create: null pointer");
    if (ntaps < 1 || ntaps > 4096) return nsh::fail_msg("nsh_fft_filter_plan_create: ntaps must be in [1, 4096]");
    for (int i = 0; i < 2 * ntaps; ++i)
        if (!std::isfinite(taps_host[i])) return nsh::fail_msg("nsh_fft_filter_plan_create: tap is not finite");
    if (fft_size != 0 && fft_size != 1024 && fft_size != 2048 && fft_size != 4096 && fft_size != 8192)
        return nsh::fail_msg("nsh_fft_filter_plan_create: fft_size must be 0, 1024, 2048, 4096 or 8192");
    if (fft_size && ntaps > fft_size / 2)
        return nsh::fail_msg("nsh_fft_filter_plan_create: ntaps must be at most fft_size / 2");
    const int N = fft_size ? fft_size : default_fft_size(ntaps);
    auto p = std::make_unique<filter_plan>();
    p->dev = dev;
    p->n = N;
    p->L = ntaps;
    p->cap_default = p->cap = default_cap(N);
    p->kernel = "k_fft_filter<" + std::to_string(N) + ">";
    const std::vector<float2> spectrum = spectrum_of(taps_host, ntaps, N);
    std::vector<float2> ordered;
    switch (N) {
    case 1024: setup<1024>(p.get(), spectrum, ordered); break;
    case 2048: setup<2048>(p.get(), spectrum, ordered); break;
    case 4096: setup<4096>(p.get(), spectrum, ordered); break;
    default: setup<8192>(p.get(), spectrum, ordered); break;
    }
    const std::vector<float2> twh = nsh::fft::pass_tables(N);
    NSH_CK(hipSetDevice(dev));
    NSH_CK(hipMalloc(&p->tw, twh.size() * sizeof(float2)));
    NSH_CK(hipMemcpy(p->tw, twh.data(), twh.size() * sizeof(float2), hipMemcpyHostToDevice));
    NSH_CK(hipMalloc(&p->hs, ordered.size() * sizeof(float2)));
    NSH_CK(hipMemcpy(p->hs, ordered.data(), ordered.size() * sizeof(float2), hipMemcpyHostToDevice));
    *plan = p.release();
    return 0;
}

int nsh_fft_filter_plan_destroy(void* plan)
{
    delete static_cast<filter_plan*>(plan);
    return 0;
}

int nsh_fft_filter_fft_size(void* plan) { return plan ? static_cast<filter_plan*>(plan)->n : 0; }
int nsh_fft_filter_valid(void* plan)
{
    const auto* p = static_cast<const filter_plan*>(plan);
    return p ? p->n - (p->L - 1) : 0;
}
int nsh_fft_filter_history(void* plan) { return plan ? static_cast<filter_plan*>(plan)->L - 1 : 0; }
int nsh_fft_filter_tile(void* plan) { return plan ? static_cast<filter_plan*>(plan)->tile : 0; }
const char* nsh_fft_filter_kernel(void* plan) { return plan ? static_cast<filter_plan*>(plan)->kernel.c_str() : ""; }

int nsh_fft_filter_grid_cap(void* plan, int max_workgroups)
{
    if (max_workgroups < 0) return nsh::fail_msg("nsh_fft_filter_grid_cap: negative cap");
    if (!plan) return nsh::fail_msg("nsh_fft_filter_grid_cap: null plan");
    auto* p = static_cast<filter_plan*>(plan);
    p->cap = max_workgroups ? max_workgroups : p->cap_default;
    return 0;
}

int nsh_fft_filter_ccc(void* plan, const float* in, const float* hist_in, float* hist_out, float* out, int64_t n, void* stream)
{
    nsh::launch_events_guard timing_guard; // an armed event pair never outlives this call
    if (n <= 0) return 0;
    if (!in || !out) return nsh::fail_msg("nsh_fft_filter_ccc: null input or output");
    if (in == out) return nsh::fail_msg("nsh_fft_filter_ccc: in-place not supported");
    if (hist_in && hist_in == hist_out) return nsh::fail_msg("nsh_fft_filter_ccc: hist_out must not alias hist_in");
    if (!plan) return nsh::fail_msg("nsh_fft_filter_ccc: null plan");
    const auto* p = static_cast<const filter_plan*>(plan);
    if (!hist_out && p->L > 1) return nsh::fail_msg("nsh_fft_filter_ccc: hist_out is required (ntaps-1 samples)");
    if (n > INT64_MAX / 16) return nsh::fail_msg("nsh_fft_filter_ccc: too many samples for one call");
    const int V = p->n - (p->L - 1);
    const int64_t nframes = (n + V - 1) / V;
    p->launch(p, (const float2*)in, (const float2*)hist_in, (float2*)hist_out, (float2*)out, n,
              nsh::fft::frame_grid(nframes, p->tile, p->cap), nsh::S(stream));
    NSH_CK_LAUNCH("nsh_fft_filter_ccc");
    return 0;
}

} // extern "C"
