// libnsh_hip.so: plan-based complex FFT of N = 2^k points, 16 <= N <= 8192 (fft_vcc: forward or
// inverse, unnormalised, an optional real window on the input and an optional half-frame shift),
// one launch, every sample over HBM once each way.
//
//   forward  X[k] = sum_n x[n] w[n] e^{-2 pi i kn/N};  shift: out[k] = X[k ^ N/2]
//   inverse  y[n] = x[n] w[n];  shift: y'[n] = y[n ^ N/2];  out[m] = sum_n y'[n] e^{+2 pi i mn/N}
//
// Stockham autosort, every lane owning 16 samples, a team of TT = max(64, N/16) lanes owning
// S = 16 TT = max(1024, N) samples, i.e. S / N whole frames (N <= 1024: one wave, 1024 / N frames)
// or one frame across N / 1024 waves (N >= 2048). The radix plan is 16 while 16 divides what is
// left, then the rest (2, 4 or 8): 16 -> {16}, 64 -> {16, 4}, 512 -> {16, 16, 2}, 8192 ->
// {16, 16, 16, 2}. A pass of radix R over sub-transforms of Ns points gives each lane 16 / R
// butterflies; butterfly b = t + TT i of the team is butterfly j = b mod (N / R) of frame
// b / (N / R):
//   reads   src[j + (N / R) r]                      r < R
//   twiddle W_{Ns R}^{(j mod Ns) r}
//   writes  dst[(j - j mod Ns) R + (j mod Ns) + Ns r]
// Pass 1 (Ns = 1) takes its input from the registers the frame was loaded into, the last pass
// leaves its output in registers for the store; the passes between exchange through the team's
// padded LDS image (one pad sample per 16), with wave barriers for one-wave teams and LDS-only
// workgroup barriers for the others. The twiddles of pass (Ns, R) are a table of (R - 1) Ns
// entries in the order the lanes read them, T[r - 1][k] = W_{Ns R}^{k r}: consecutive lanes,
// consecutive entries. All tables of a size (fewer than N entries together) are computed in double
// on the host and staged in LDS once per workgroup.
//
// The window is one fp32 multiply per component as the samples leave the load registers; a lane
// meets the same 16 window entries in every frame, so they are loaded once per kernel (1.0 without a
// window: an exact multiply). The shift is index ^ N/2 on the store (forward) or the load (inverse).
// N = 1024 without window and shift runs k_fft1024 (nsh_fft.hip).
// The geometry, the passes and fft_team are in nsh_fft_team.hpp (k_fft_xlat uses them too).
#include "nsh_fft_team.hpp"

#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

namespace {

using nsh::cf;
using nsh::fft::fft_team;
using nsh::fft::geom;
using nsh::fft::pad;
using nsh::fft::pass_tables;
using nsh::fft::team_sync;
using nsh::fft::to_device;

// LIN (N <= 1024): every global access is the wave's coalesced walk (sample t + 64 m), and the
// registers of pass 1 and of the last pass are filled from / emptied into the image by a
// transposing LDS access. Without it lane t loads in_idx(t, r): runs of N / 16 consecutive samples,
// i.e. 8 bytes per lane at a 128-byte stride for N = 16 (DESIGN 4.7 has the measurement).
template <int N, bool INV, bool LIN>
__global__ __launch_bounds__(geom<N>::NT) void k_fft(const float2* __restrict__ in, float2* __restrict__ out, int64_t nframes,
                                                     const float2* __restrict__ tw_g, const float* __restrict__ win, int ldx,
                                                     int stx)
{
    using G = geom<N>;
    static_assert(!LIN || G::TT == 64, "linear I/O is for one-wave teams");
    constexpr bool USE_IMG = N > 16 || LIN;
    __shared__ cf tw[G::TWN ? G::TWN : 1];
    __shared__ cf img_all[USE_IMG ? G::TEAMS * G::IMG : 1];
    nsh::fft::stage_table(tw, tw_g, G::TWN, threadIdx.x, G::NT);
    __syncthreads();
    const int t = threadIdx.x & (G::TT - 1), team = threadIdx.x / G::TT;
    cf* img = img_all + (USE_IMG ? team * G::IMG : 0);
    // sample of the chunk in load register m / store register m (before the shift's xor)
    const auto ld_idx = [t, ldx](int m) { return (LIN ? t + 64 * m : G::in_idx(t, m)) ^ ldx; };
    const auto st_idx = [t, stx](int m) { return (LIN ? t + 64 * m : G::out_idx(t, m)) ^ stx; };
    float wv[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) wv[m] = win ? win[ld_idx(m) & (N - 1)] : 1.f;

    // every team of the workgroup walks the same number of steps (workgroup barriers inside): a team
    // past the end loads zeros and its stores are dropped
    const int64_t total = nframes * N;
    const int64_t ngroups = (nframes + G::TILE - 1) / G::TILE;
    int64_t g = blockIdx.x;
    if (g >= ngroups) return;
    cf v[16], nx[16];
    nsh::fft::load16<G::S>(v, in, g * G::TEAMS + team, total, ld_idx);
    for (; g < ngroups; g += gridDim.x) {
        nsh::fft::load16<G::S>(nx, in, (g + gridDim.x) * G::TEAMS + team, total, ld_idx);
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] *= wv[m];
        if constexpr (LIN) {
#pragma unroll
            for (int m = 0; m < 16; ++m) img[pad(t + 64 * m)] = v[m];
            team_sync<false>();
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = img[pad(G::in_idx(t, r))];
            team_sync<false>();
        }
        fft_team<N, INV>(v, img, tw, t);
        if constexpr (LIN) {
#pragma unroll
            for (int m = 0; m < 16; ++m) img[pad(G::out_idx(t, m))] = v[m];
            team_sync<false>();
#pragma unroll
            for (int m = 0; m < 16; ++m) v[m] = img[pad(t + 64 * m)];
            team_sync<false>();
        }
        nsh::fft::store16<G::S>(v, out, g * G::TEAMS + team, total, st_idx);
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = nx[m];
    }
}

struct fft_plan {
    int dev = 0, n = 0, tile = 0, cap = 0, cap_default = 0;
    bool inverse = false, shift = false, plain1024 = false;
    float2* tw = nullptr;
    float* win = nullptr;
    std::string kernel;
    void (*launch)(const fft_plan*, const float2*, float2*, int64_t, unsigned, hipStream_t) = nullptr;
    ~fft_plan()
    {
        nsh::dev_free(tw);
        nsh::dev_free(win);
    }
};

template <int N, bool INV, bool LIN>
void launch_fft(const fft_plan* p, const float2* in, float2* out, int64_t nframes, unsigned grid, hipStream_t s)
{
    nsh::launch((k_fft<N, INV, LIN>), dim3(grid), dim3(geom<N>::NT), 0, s, in, out, nframes, (const float2*)p->tw,
                (const float*)p->win, p->shift && p->inverse ? N / 2 : 0, p->shift && !p->inverse ? N / 2 : 0);
}

// Workgroups of the grid-stride walk. A workgroup stages its size's twiddle tables once (about N
// entries against the 4096 or 8192 samples of a tile) and prefetches only from its second tile on,
// so at 2^26 samples one tile per workgroup (16384 workgroups) costs 170 -> 188 us at N = 64,
// 171 -> 249 us at 2048 and 213 -> 295 us at 8192 against the caps below, the best of a sweep over
// 512 .. 16384 (tools/fft_bench.py --cap-sweep); fewer, longer workgroups lose again
// (N <= 1024: 178 us at 512).
constexpr int default_cap(int n) { return n <= 1024 ? 8192 : n <= 4096 ? 2048 : 1024; }
// sizes up to this one move their samples by linear accesses through the image (k_fft's LIN):
// 168 against 1445 us per 2^26 samples at N = 16, 167 / 336 at 32, 166 / 216 at 64, 167 / 176 at 128,
// 166 / 168 (within the spread) at 256 (tools/fft_bench.py --io-ab, profiles/fft_bench.json)
constexpr int LIN_MAX = 128;
constexpr int LIN_INST_MAX = 256; // ... and the largest size that instantiates it at all

template <int N>
void setup(fft_plan* p, bool lin)
{
    p->tile = geom<N>::TILE;
    if constexpr (N <= LIN_INST_MAX) {
        if (lin) {
            p->launch = p->inverse ? launch_fft<N, true, true> : launch_fft<N, false, true>;
            return;
        }
    }
    p->launch = p->inverse ? launch_fft<N, true, false> : launch_fft<N, false, false>;
}

} // namespace

extern "C" {

int nsh_fft_plan_create(int dev, int fft_size, int inverse, const float* window_host, int shift, void** plan)
{
    if (!plan) return nsh::fail_msg("nsh_fft_plan_create: null pointer");
    if (fft_size < 16 || fft_size > 8192 || (fft_size & (fft_size - 1)))
        return nsh::fail_msg("nsh_fft_plan_create: fft_size must be a power of two in [16, 8192]");
    if (window_host)
        for (int i = 0; i < fft_size; ++i)
            if (!std::isfinite(window_host[i])) return nsh::fail_msg("nsh_fft_plan_create: window entry is not finite");
    auto p = std::make_unique<fft_plan>();
    p->dev = dev;
    p->n = fft_size;
    p->inverse = inverse != 0;
    p->shift = shift != 0;
    p->plain1024 = fft_size == 1024 && !window_host && !shift;
    p->cap_default = p->cap = p->plain1024 ? 0 : default_cap(fft_size); // 0: k_fft1024's own (FFT_CAP)
    // NSH_FFT_IO=strided|linear overrides the size threshold (the A/B of tools/fft_bench.py)
    bool lin = fft_size <= LIN_MAX && fft_size <= LIN_INST_MAX;
    if (const char* e = std::getenv("NSH_FFT_IO")) {
        if (std::string(e) == "linear") lin = fft_size <= LIN_INST_MAX;
        if (std::string(e) == "strided") lin = false;
    }
    switch (fft_size) {
    case 16: setup<16>(p.get(), lin); break;
    case 32: setup<32>(p.get(), lin); break;
    case 64: setup<64>(p.get(), lin); break;
    case 128: setup<128>(p.get(), lin); break;
    case 256: setup<256>(p.get(), lin); break;
    case 512: setup<512>(p.get(), lin); break;
    case 1024: setup<1024>(p.get(), lin); break;
    case 2048: setup<2048>(p.get(), lin); break;
    case 4096: setup<4096>(p.get(), lin); break;
    default: setup<8192>(p.get(), lin); break;
    }
    if (p->plain1024) {
        p->tile = 4;
        p->kernel = std::string("k_fft1024<") + (p->inverse ? "true>" : "false>");
    } else
        p->kernel = "k_fft<" + std::to_string(fft_size) + (p->inverse ? ", true, " : ", false, ") +
                    (lin ? "true>" : "false>");
    if (!p->plain1024) {
        NSH_CK(hipSetDevice(dev));
        if (const int rc = to_device(pass_tables(fft_size), &p->tw)) return rc;
        if (window_host)
            if (const int rc = to_device(std::vector<float>(window_host, window_host + fft_size), &p->win)) return rc;
    }
    *plan = p.release();
    return 0;
}

int nsh_fft_plan_destroy(void* plan)
{
    delete static_cast<fft_plan*>(plan);
    return 0;
}

int nsh_fft_plan_size(void* plan) { return plan ? static_cast<fft_plan*>(plan)->n : 0; }
int nsh_fft_tile(void* plan) { return plan ? static_cast<fft_plan*>(plan)->tile : 0; }
const char* nsh_fft_kernel(void* plan) { return plan ? static_cast<fft_plan*>(plan)->kernel.c_str() : ""; }

int nsh_fft_plan_grid_cap(void* plan, int max_workgroups)
{
    if (max_workgroups < 0) return nsh::fail_msg("nsh_fft_plan_grid_cap: negative cap");
    if (!plan) return nsh::fail_msg("nsh_fft_plan_grid_cap: null plan");
    auto* p = static_cast<fft_plan*>(plan);
    p->cap = max_workgroups ? max_workgroups : p->cap_default;
    return 0;
}

int nsh_fft_c2c(void* plan, const float* in, float* out, int64_t nframes, void* stream)
{
    nsh::launch_events_guard timing_guard; // an armed event pair never outlives this call
    if (nframes <= 0) return 0;
    if (!in || !out) return nsh::fail_msg("nsh_fft_c2c: null pointer");
    if (in == out) return nsh::fail_msg("nsh_fft_c2c: in-place not supported");
    if (!plan) return nsh::fail_msg("nsh_fft_c2c: null plan");
    const auto* p = static_cast<const fft_plan*>(plan);
    if (nframes > INT64_MAX / 8 / p->n) return nsh::fail_msg("nsh_fft_c2c: nframes too large");
    if (p->plain1024)
        return nsh::fft::fft1024_launch((const float2*)in, (float2*)out, nframes, p->inverse, p->cap, nsh::S(stream),
                                        "nsh_fft_c2c");
    p->launch(p, (const float2*)in, (float2*)out, nframes, nsh::fft::frame_grid(nframes, p->tile, p->cap), nsh::S(stream));
    NSH_CK_LAUNCH("nsh_fft_c2c");
    return 0;
}

} // extern "C"
