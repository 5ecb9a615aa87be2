// libnsh_hip.so: psd_vcf, the spectrum estimate fft_vcc -> complex_to_mag_squared -> integrate_ff
// (-> nlog10_ff) in one launch: every complex sample is read once, N floats leave per K frames.
//
//   X_f[k]  = sum_n x_f[n] w[n] e^{-2 pi i kn/N}       frame f = samples fN .. fN+N-1, as k_fft<N, false>
//   P_j[k]  = scale sum_{f = jK .. jK+K-1} |X_f[k]|^2
//   out_j[k] = P_j[k ^ (shift ? N/2 : 0)],  or 10 log10f of it (db)
//
// Rows. The K frames of output vector j are cut into nseg = ceil(K / P) segments of P frames (the
// last may be shorter); a row is one segment of one vector, row r = j nseg + seg, its frames
// contiguous in memory. A team step (geom<N>, nsh_fft_team.hpp) transforms F frames as k_fft does,
// but they are frame s of F different rows, so register m of a lane meets the same (row, bin) in
// every step and the sum over a row's frames is acc[m] += re^2 + im^2 in registers: no cross-lane
// fold, no LDS beyond the transform's, any K. A workgroup owns TILE = TEAMS F consecutive rows and
// walks min(P, K) steps over them; rows past the end and steps past a short row's end load zeros,
// which add exactly 0. The sum of a vector is therefore the same chain of fp32 additions wherever
// the vector lies in a call: frames in order within a segment, then the segments (k_psd_sum).
//
// nseg = 1: a row is a vector; its sums are scaled, optionally logged and stored to out, the shift
// as ^ N/2 on the store index. nseg > 1: rows go to the plan's scratch [row][N] and k_psd_sum adds
// each vector's segments in a fixed order (k_psd_sum), scales, logs and stores. A call with more rows than the
// scratch holds proceeds in batches of whole vectors; the scratch makes a plan serve one stream at
// a time.
//
// Loads. A team's F rows start up to F K N samples apart (at most 2^29 bytes, F N = 1024 for
// F > 1), so one buffer resource per team and step, based at frame s of the team's first row and
// reaching to the end of the input (clamped below 2^31), addresses all of them with a per-lane
// 32-bit offset; a lane whose row has ended, or does not exist, gets an offset past every resource
// and reads zeros. The loop issues the same 16 loads every step, so the next step's stay in flight
// across this step's transform. LIN (N <= 128, as k_fft in nsh_fft_plan.hip): lanes walk each
// frame's N-sample piece linearly and the registers are transposed through the team's image before
// and after the transform.
#include "nsh_fft_team.hpp"

#include <cmath>
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

// bytes from base on, at most kSpan; built from wave-uniform values only (chunk_rsrc)
constexpr int64_t kSpan = 0x70000000;
// a byte offset past every resource of this kernel, far from wrapping
constexpr int kNowhere = 0x7ffffff0;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t bytes_rsrc(const void* base, int64_t bytes)
{
    bytes = bytes < 0 ? 0 : (bytes > kSpan ? kSpan : bytes);
    const uint64_t a = (uint64_t)base;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    const int b = __builtin_amdgcn_readfirstlane((int)bytes);
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), (short)0, b, 0x00020000);
}

enum { PSD_PARTIAL = 0, PSD_LINEAR = 1, PSD_DB = 2 };

__device__ __forceinline__ float finish(float sum, float scale, int mode)
{
    const float p = sum * scale;
    return mode == PSD_DB ? 10.f * log10f(p) : p;
}

// in: the batch's first sample, frames frames of N follow. dst: out (mode != PSD_PARTIAL, nseg = 1,
// row = vector) or the scratch (PSD_PARTIAL), [nrows][N]. stx: N/2 for a shifted store to out.
// (two waves per SIMD: without the request N = 128 takes 259 registers and runs one)
template <int N, bool LIN>
__global__ __launch_bounds__(geom<N>::NT) __attribute__((amdgpu_waves_per_eu(2))) void k_psd(
    const float2* __restrict__ in, float* __restrict__ dst, int nrows, int K, int P, int nseg, int64_t frames,
    const float2* __restrict__ tw_g, const float* __restrict__ win, int stx, float scale, int mode)
{
    using G = geom<N>;
    static_assert(!LIN || G::TT == 64, "linear I/O is for one-wave teams");
    constexpr bool USE_IMG = N > 16 || LIN;
    constexpr int NQ = LIN ? 16 : 1; // rows a lane's load registers meet
    __shared__ cf tw[G::TWN ? G::TWN : 1];
    __shared__ cf img_all[USE_IMG ? G::TEAMS * G::IMG : 1];
    nsh::fft::stage_table(tw, tw_g, G::TWN, threadIdx.x, G::NT);
    __syncthreads();
    const int t = threadIdx.x & (G::TT - 1), team = threadIdx.x / G::TT;
    cf* img = img_all + (USE_IMG ? team * G::IMG : 0);
    // sample of the team's F frames (frame slot q = idx / N, sample idx % N) in load register m /
    // accumulator m
    const auto ld_idx = [t](int m) { return LIN ? t + 64 * m : G::in_idx(t, m); };
    const auto st_idx = [t](int m) { return LIN ? t + 64 * m : G::out_idx(t, m); };
    float wv[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) wv[m] = win ? win[ld_idx(m) & (N - 1)] : 1.f;

    const int steps = K < P ? K : P;
    const int ngroups = (nrows + G::TILE - 1) / G::TILE;
    // Rows of group g for this lane: rel[d] frames from the team's first row's first frame (start0) to
    // the first frame of the row of load registers d (LIN: register d; else all 16), len[d] its frames
    // (0 for a row past the end)
    int rel[NQ], len[NQ];
    int64_t start0;
    const auto describe = [&](int g) {
        const int r0 = (g * G::TEAMS + team) * G::F;
        const int vec0 = nseg == 1 ? r0 : r0 / nseg, seg0 = r0 - vec0 * nseg;
        start0 = (int64_t)vec0 * K + seg0 * P;
#pragma unroll
        for (int d = 0; d < NQ; ++d) {
            // frame slot of sample t + 64 d (N divides 64, or t < 64 <= N and 64 d mod N + t < N)
            const int q = LIN ? (N < 64 ? t / N : 0) + (64 * d) / N : (G::F > 1 ? t / (N / 16) : 0);
            const int r = r0 + q;
            const int vec = nseg == 1 ? r : r / nseg, seg = r - vec * nseg;
            rel[d] = (vec - vec0) * K + (seg - seg0) * P;
            const int left = K - seg * P;
            len[d] = r < nrows ? (left < P ? left : P) : 0;
        }
    };
    // frame s of the team's rows
    const auto load_step = [&](cf(&v)[16], int s) {
        const int64_t f0 = start0 + s, left = frames - f0;
        const __amdgpu_buffer_rsrc_t r = bytes_rsrc(in + (left > 0 ? f0 * N : 0), left * (N * 8));
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const int d = LIN ? m : 0;
            const int off = s < len[d] ? (rel[d] * N + (ld_idx(m) & (N - 1))) * 8 : kNowhere;
            v[m] = __builtin_bit_cast(cf, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, nsh::AUX_LD));
        }
    };

    // every team of the workgroup walks the same (group, step) sequence (workgroup barriers inside)
    int g = blockIdx.x, s = 0;
    if (g >= ngroups) return;
    float acc[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) acc[m] = 0.f;
    cf v[16], nx[16];
    describe(g);
    load_step(v, 0);
    while (g < ngroups) {
        const bool last = s + 1 == steps;
        const int ng = last ? g + (int)gridDim.x : g, ns = last ? 0 : s + 1;
        const int r0 = (g * G::TEAMS + team) * G::F; // before describe() moves on
        if (last) describe(ng);
        load_step(nx, ns);
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
        fft_team<N, false>(v, img, tw, t);
        if constexpr (LIN) {
#pragma unroll
            for (int m = 0; m < 16; ++m) img[pad(G::out_idx(t, m))] = v[m];
            team_sync<false>();
#pragma unroll
            for (int m = 0; m < 16; ++m) v[m] = img[pad(t + 64 * m)];
            team_sync<false>();
        }
#pragma unroll
        for (int m = 0; m < 16; ++m) acc[m] += v[m].x * v[m].x + v[m].y * v[m].y;
        if (last) {
            int rows = nrows - r0;
            rows = rows < 0 ? 0 : (rows > G::F ? G::F : rows);
            const __amdgpu_buffer_rsrc_t r = bytes_rsrc(dst + (rows > 0 ? (int64_t)r0 * N : 0), (int64_t)rows * (N * 4));
            if (mode != PSD_PARTIAL) {
#pragma unroll
                for (int m = 0; m < 16; ++m) acc[m] *= scale;
            }
            if (mode == PSD_DB) {
#pragma unroll
                for (int m = 0; m < 16; ++m) acc[m] = 10.f * log10f(acc[m]);
            }
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, acc[m]), r, (st_idx(m) ^ stx) * 4, 0,
                                                      nsh::AUX_ST);
                acc[m] = 0.f;
            }
        }
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = nx[m];
        g = ng;
        s = ns;
    }
}

// out[vec][k ^ stx] = finish(sum over the vector's nseg rows of part[row][k]). A workgroup owns
// B = 2^lgb bins of one vector; its 256 / B groups of lanes add the rows g, g + G, g + 2G, .. each in
// that order, and the groups' sums are added in group order: a chain that depends on (nseg, B)
// alone. (One lane per bin adding all rows is a chain of nseg dependent loads: 1.7 ms for the 4096
// rows of one 65536-frame spectrum at P = 16.)
__global__ __launch_bounds__(256) void k_psd_sum(const float* __restrict__ part, float* __restrict__ out, int lgn, int nseg,
                                                 int lgb, int stx, float scale, int mode)
{
    __shared__ float red[256];
    const int G = 256 >> lgb, kk = threadIdx.x & ((1 << lgb) - 1), grp = threadIdx.x >> lgb;
    const int64_t vec = blockIdx.x >> (lgn - lgb);
    const int k = (int)((blockIdx.x & ((1u << (lgn - lgb)) - 1)) << lgb) + kk;
    const float* p = part + ((vec * nseg) << lgn) + k;
    float sum = 0.f; // 0 + x = x: the sums are not negative
#pragma unroll 8
    for (int r = grp; r < nseg; r += G) sum += p[(int64_t)r << lgn];
    red[threadIdx.x] = sum;
    __syncthreads();
    if (grp == 0) {
        for (int g = 1; g < G; ++g) sum += red[(g << lgb) + kk];
        out[(vec << lgn) + (k ^ stx)] = finish(sum, scale, mode);
    }
}

struct psd_plan {
    int dev = 0, n = 0, lgn = 0, navg = 0, seg = 0, nseg = 0, tile = 0, cap = 0, cap_default = 0;
    int lgb = 0; // k_psd_sum: log2 of the bins of a workgroup
    bool shift = false, db = false;
    float scale = 1.f;
    float2* tw = nullptr;
    float* win = nullptr;
    float* part = nullptr; // [part_rows][n], nseg > 1
    int64_t part_rows = 0;
    std::string kernel;
    void (*launch)(const psd_plan*, const float2*, float*, int, int64_t, int, int, unsigned, hipStream_t, hipEvent_t,
                   hipEvent_t) = nullptr;
    ~psd_plan()
    {
        nsh::dev_free(tw);
        nsh::dev_free(win);
        nsh::dev_free(part);
    }
};

template <int N, bool LIN>
void launch_psd(const psd_plan* p, const float2* in, float* dst, int nrows, int64_t frames, int stx, int mode, unsigned grid,
                hipStream_t s, hipEvent_t start, hipEvent_t stop)
{
    nsh::launch_timed((k_psd<N, LIN>), dim3(grid), dim3(geom<N>::NT), 0, s, start, stop, in, dst, nrows, p->navg, p->seg, p->nseg,
                      frames, (const float2*)p->tw, (const float*)p->win, stx, p->scale, mode);
}

// Most frames of a segment: K frames are cut into nseg = ceil(K / kSegment) segments of
// P = ceil(K / nseg) frames, so every row walks P steps and at most nseg - 1 of a vector's nseg P
// steps transform zeros (K = 33: 17 + 16 frames, not 32 + 1). NSH_PSD_SEGMENT overrides kSegment
// at plan creation (the sweep of tools/psd_bench.py); 0 there means no segmentation. Short segments cost
// scratch traffic (4 / P bytes a sample each way), long ones leave a long average of few vectors
// with too few rows to fill the GPU. us per 2^26 samples at P = 4 / 8 / 16 / 32 / 64 / 256
// (tools/psd_bench.py --sweep, profiles/psd_bench.json):
//   N = 64:   K = 1024 (1024 vectors) 141 / 127 / 113 / 106 / 129 / 435, K = 65536 (16) 200 / 155 / 125 / 110 / 125 / 416
//   N = 1024: K = 1024 (64) 133 / 119 / 113 / 107 / 131 / 447, K = 65536 (1) 194 / 148 / 127 / 113 / 128 / 438
//   N = 4096: K = 1024 (16) 161 / 149 / 142 / 135 / 181 / 636, K = 16384 (1) 161 / 149 / 142 / 137 / 181 / 638
//   N = 8192: K = 1024 (8) 211 / 198 / 192 / 189 / 330 / 1200, K = 8192 (1) 210 / 198 / 191 / 189 / 331 / 1200
// and 1.6 to 106 ms without segmentation (P = K).
constexpr int kSegment = 32;
// Workgroups of the grid-stride walk over row groups. A workgroup stages its size's twiddle tables
// once, describes its rows once per group and prefetches from its second step on; us per 2^26
// samples at K = 1 under caps of 256 / 512 / 1024 / 2048 / 4096 / 8192 / 16384 (the same sweep):
//   N = 64:   157 / 137 / 136 / 135 / 137 / 152 / 187      N = 1024: 145 / 136 / 134 / 132 / 134 / 141 / 181
//   N = 4096: 179 / 143 / 144 / 152 / 165 / 191 / 269      N = 8192: 198 / 200 / 206 / 217 / 242 / 309 / 308
// K = 16 and the single-spectrum shapes are level from 512 on (N <= 4096) and 2 % better at 256 (8192).
constexpr int default_cap(int n) { return n <= 1024 ? 2048 : n <= 4096 ? 512 : 256; }
// sizes up to this one run LIN: k_fft's threshold (nsh_fft_plan.hip, measured in DESIGN 4.7)
constexpr int kLinMax = 128;
// bytes of scratch a plan with nseg > 1 owns (at least one vector's rows); NSH_PSD_SCRATCH_BYTES
// overrides it at plan creation
constexpr int64_t kScratchBytes = 64 << 20;
// rows of one launch: row indices and their products with TILE stay in int
constexpr int64_t kMaxRows = 1 << 28;
// vectors of one k_psd_sum launch: at most 512 workgroups each
constexpr int64_t kMaxSumVectors = 1 << 20;

template <int N>
void setup(psd_plan* p)
{
    constexpr bool LIN = N <= kLinMax;
    p->tile = geom<N>::TILE;
    p->launch = launch_psd<N, LIN>;
    p->kernel = "k_psd<" + std::to_string(N) + (LIN ? ", true>" : ", false>");
}

int64_t env_int(const char* name, int64_t dflt)
{
    const char* e = std::getenv(name);
    if (!e || !*e) return dflt;
    char* end = nullptr;
    const long long v = std::strtoll(e, &end, 10);
    return end && *end == 0 && v >= 0 ? (int64_t)v : dflt;
}

} // namespace

extern "C" {

int nsh_psd_plan_create(int dev, int fft_size, int navg, const float* window_host, int shift, float scale, int db, void** plan)
{
    if (!plan) return nsh::fail_msg("nsh_psd_plan_create: null pointer");
    if (fft_size < 16 || fft_size > 8192 || (fft_size & (fft_size - 1)))
        return nsh::fail_msg("nsh_psd_plan_create: fft_size must be a power of two in [16, 8192]");
    if (navg < 1 || navg > 65536) return nsh::fail_msg("nsh_psd_plan_create: navg must be in [1, 65536]");
    if (window_host)
        for (int i = 0; i < fft_size; ++i)
            if (!std::isfinite(window_host[i])) return nsh::fail_msg("nsh_psd_plan_create: window entry is not finite");
    if (!std::isfinite(scale) || !(scale > 0.f)) return nsh::fail_msg("nsh_psd_plan_create: scale must be finite and > 0");
    auto p = std::make_unique<psd_plan>();
    p->dev = dev;
    p->n = fft_size;
    while ((1 << p->lgn) < fft_size) ++p->lgn;
    p->navg = navg;
    p->shift = shift != 0;
    p->db = db != 0;
    p->scale = scale;
    int64_t seg = env_int("NSH_PSD_SEGMENT", kSegment);
    if (seg < 1 || seg > navg) seg = navg;
    p->nseg = (navg + (int)seg - 1) / (int)seg;
    p->seg = (navg + p->nseg - 1) / p->nseg; // nseg = ceil(navg / seg) still holds
    p->cap_default = p->cap = default_cap(fft_size);
    switch (fft_size) {
    case 16: setup<16>(p.get()); break;
    case 32: setup<32>(p.get()); break;
    case 64: setup<64>(p.get()); break;
    case 128: setup<128>(p.get()); break;
    case 256: setup<256>(p.get()); break;
    case 512: setup<512>(p.get()); break;
    case 1024: setup<1024>(p.get()); break;
    case 2048: setup<2048>(p.get()); break;
    case 4096: setup<4096>(p.get()); break;
    default: setup<8192>(p.get()); break;
    }
    NSH_CK(hipSetDevice(dev));
    if (const int rc = to_device(pass_tables(fft_size), &p->tw)) return rc;
    if (window_host)
        if (const int rc = to_device(std::vector<float>(window_host, window_host + fft_size), &p->win)) return rc;
    if (p->nseg > 1) {
        const int64_t row_bytes = (int64_t)fft_size * 4;
        int64_t vecs = env_int("NSH_PSD_SCRATCH_BYTES", kScratchBytes) / (row_bytes * p->nseg);
        if (vecs < 1) vecs = 1;
        if (vecs * p->nseg > kMaxRows) vecs = kMaxRows / p->nseg;
        if (vecs > kMaxSumVectors) vecs = kMaxSumVectors;
        // up to 16 groups of lanes share a vector's rows, at least 16 bins (64 bytes of a row) a group
        int groups = 1;
        while (groups < 16 && groups < p->nseg) groups *= 2;
        const int bins = 256 / groups < fft_size ? 256 / groups : fft_size;
        while ((1 << p->lgb) < bins) ++p->lgb;
        p->part_rows = vecs * p->nseg;
        NSH_CK(hipMalloc(&p->part, p->part_rows * row_bytes));
    }
    *plan = p.release();
    return 0;
}

int nsh_psd_plan_destroy(void* plan)
{
    delete static_cast<psd_plan*>(plan);
    return 0;
}

int nsh_psd_fft_size(void* plan) { return plan ? static_cast<psd_plan*>(plan)->n : 0; }
int nsh_psd_navg(void* plan) { return plan ? static_cast<psd_plan*>(plan)->navg : 0; }
int nsh_psd_segment(void* plan) { return plan ? static_cast<psd_plan*>(plan)->seg : 0; }
int nsh_psd_tile(void* plan) { return plan ? static_cast<psd_plan*>(plan)->tile : 0; }
const char* nsh_psd_kernel(void* plan) { return plan ? static_cast<psd_plan*>(plan)->kernel.c_str() : ""; }

int nsh_psd_grid_cap(void* plan, int max_workgroups)
{
    if (max_workgroups < 0) return nsh::fail_msg("nsh_psd_grid_cap: negative cap");
    if (!plan) return nsh::fail_msg("nsh_psd_grid_cap: null plan");
    auto* p = static_cast<psd_plan*>(plan);
    p->cap = max_workgroups ? max_workgroups : p->cap_default;
    return 0;
}

int nsh_psd_cf(void* plan, const float* in, float* out, int64_t nvec, void* stream)
{
    nsh::launch_events_guard timing_guard; // an armed event pair never outlives this call
    if (nvec <= 0) return 0;
    if (!in || !out) return nsh::fail_msg("nsh_psd_cf: null pointer");
    if ((const void*)in == (const void*)out) return nsh::fail_msg("nsh_psd_cf: in-place not supported");
    if (!plan) return nsh::fail_msg("nsh_psd_cf: null plan");
    const auto* p = static_cast<const psd_plan*>(plan);
    if (nvec > INT64_MAX / 8 / p->n / p->navg) return nsh::fail_msg("nsh_psd_cf: nvec too large");
    // one pair for the whole call: start with the first launch, stop with the last
    const nsh::launch_events ev = nsh::take_launch_events();
    const hipStream_t s = nsh::S(stream);
    const int mode = p->db ? PSD_DB : PSD_LINEAR, stx = p->shift ? p->n / 2 : 0;
    const int64_t per = p->nseg > 1 ? p->part_rows / p->nseg : kMaxRows; // vectors of a batch
    for (int64_t v0 = 0; v0 < nvec; v0 += per) {
        const int64_t nv = nvec - v0 < per ? nvec - v0 : per;
        const bool first = v0 == 0, final = v0 + nv == nvec;
        const float2* bin = (const float2*)in + v0 * p->navg * p->n;
        float* bout = out + v0 * p->n;
        const int nrows = (int)(nv * p->nseg);
        const unsigned grid = nsh::fft::frame_grid(nrows, p->tile, p->cap);
        if (p->nseg == 1) {
            p->launch(p, bin, bout, nrows, nv * p->navg, stx, mode, grid, s, first ? ev.start : nullptr, final ? ev.stop : nullptr);
            NSH_CK_LAUNCH("nsh_psd_cf");
        } else {
            p->launch(p, bin, p->part, nrows, nv * p->navg, 0, PSD_PARTIAL, grid, s, first ? ev.start : nullptr, nullptr);
            NSH_CK_LAUNCH("nsh_psd_cf");
            nsh::launch_timed(k_psd_sum, dim3((unsigned)(nv << (p->lgn - p->lgb))), dim3(256), 0, s, (hipEvent_t) nullptr,
                              final ? ev.stop : nullptr, (const float*)p->part, bout, p->lgn, p->nseg, p->lgb, stx, p->scale, mode);
            NSH_CK_LAUNCH("nsh_psd_cf(sum)");
        }
    }
    return 0;
}

} // extern "C"
