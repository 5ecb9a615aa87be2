// libnsh_hip.so: 1024-point complex FFT (fft_vcc forward/inverse, unnormalised) and the
// fused fft -> multiply -> ifft channelizer of BASELINE config C4.
//
// No reference counterpart (the "Num FFT Blocks" option of
// schedulers/mt/bench/cuda/bm_copy.cpp:42-43 is a mislabelled copy count). Conventions:
//   forward  X[k] = sum_n x[n] e^{-2 pi i kn/1024}            (= numpy.fft.fft)
//   inverse  x[n] = sum_k X[k] e^{+2 pi i kn/1024}            (= 1024 * numpy.fft.ifft)
//
// One wavefront per 1024-sample frame (4 frames per 256-thread workgroup, grid-stride):
// Stockham autosort in three passes, radix 16 / 16 / 4, each lane owning 16 samples:
//   pass 1 (Ns = 1):   lane j loads x[j + 64 r] (coalesced), DFT16 in registers -> LDS
//   pass 2 (Ns = 16):  reads LDS[j + 64 r], twiddles W_256^{k r}, DFT16 -> LDS
//   pass 3 (Ns = 256): 4 radix-4 butterflies per lane, twiddles W_1024^{k r} -> HBM
// DFT16 = 4 x DFT4, internal W_16 twiddles, 4 x DFT4 (index transpose at compile time). The
// LDS image (one per wave, 8.5 KiB) has one pad sample per 16 so every exchange is
// bank-conflict-free; a wave's LDS operations complete in order, so the passes need no
// workgroup barriers. Twiddles come from a 1024-entry table computed in double on the host
// and staged in LDS once per workgroup. The next frame's samples are prefetched into
// registers while the current frame transforms. The channelizer multiplies the spectrum
// by W in registers and runs the inverse transform directly: pass 3 leaves lane j holding
// indices j + 64 m (m < 16), exactly pass 1's input layout, so a frame crosses HBM once
// each way (16 B/sample instead of 48 B unfused) and LDS twice per transform.
#include "nsh_fft_shared.hpp"

#include <cmath>
#include <mutex>
#include <vector>

namespace {

constexpr int N = 1024;
constexpr int NT = 256;

using nsh::cf;
using nsh::cmulw;
using nsh::dft4;
using nsh::rot;
using nsh::fft::conj_if;
using nsh::fft::dft16;
using nsh::fft::frame_grid;
using nsh::fft::pad;

// the channelizer's spectrum multiply: nsh_mul_const_vcc's two-product rounding exactly, so
// the fused channelizer stays bit-identical to fft -> multiply_const_vcc -> ifft
__device__ __forceinline__ cf cmul_rn(cf a, cf b)
{
    const cf t = a.xx * b;    // (ax bx, ax by), each product rounded
    const cf u = a.yy * b.yx; // (ay by, ay bx)
    return t + u * cf{ -1.f, 1.f }; // (ax bx - ay by, ax by + ay bx): exact sign flip, one rounding
}
constexpr int WLDS = nsh::fft::padded(N); // one wave's padded image

// The passes' twiddles, staged per workgroup in the natural 1024-entry table. Pass 2's W_1024^{4 k r}
// (k = lane & 15) puts the 16 lanes of a read group at stride 4 r entries -- 4- to 16-way LDS bank
// conflicts (PMC: 36 % of the channelizer's LDS-active cycles are conflict cycles) -- and pass 3's
// W^{2 j'} at stride 2. Staged in the order the lanes read them instead (T2[r][k] = W^{4 k r},
// T3[r - 1][j'] = W^{r j'}) the reads are conflict-free and no faster: channelizer 765-769 vs
// 763-764 us, fft1024 707-708 vs 704 us per 2^28 samples, both orders
// (profiles/r06e_chan_twiddle_layout_ab.log) -- LDS does not bound them.
constexpr int TWN = N;
__device__ __forceinline__ void stage_twiddles(cf* __restrict__ t, const float2* __restrict__ tw_g, int tid, int nt)
{
    nsh::fft::stage_table(t, tw_g, TWN, tid, nt);
}
// pass 2's W_1024^{4 k2 r} and pass 3's W_1024^{r jp} (r = 1..3) from the staged table
template <bool INV>
__device__ __forceinline__ cf tw_pass2(const cf* __restrict__ tw, int k2, int r)
{
    return conj_if<INV>(tw[(4 * k2 * r) & (N - 1)]);
}
template <bool INV>
__device__ __forceinline__ cf tw_pass3(const cf* __restrict__ tw, int jp, int r)
{
    return conj_if<INV>(tw[(r * jp) & (N - 1)]);
}

// Transform of one frame held as v[m] = x[lane + 64 m]; on return v[m] = X[lane + 64 m]
// (pass 3 output kept in registers: m = b + 4 r for butterfly b, output r). tw: the staged table.
template <bool INV>
__device__ __forceinline__ void fft_wave(cf (&v)[16], cf* __restrict__ img, const cf* __restrict__ tw)
{
    const int j = threadIdx.x & 63;
    // pass 1: Ns = 1, radix 16 -> dst[16 j + r]
    dft16<INV>(v);
#pragma unroll
    for (int r = 0; r < 16; ++r) img[pad(16 * j + r)] = v[r];
    __builtin_amdgcn_wave_barrier();
    // pass 2: Ns = 16, radix 16: src[j + 64 r], twiddle W_256^{k r} = W_1024^{4 k r} -> dst[(j >> 4) 256 + k + 16 r]
    const int k2 = j & 15;
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = img[pad(j + 64 * r)];
#pragma unroll
    for (int r = 1; r < 16; ++r) v[r] = cmulw(v[r], tw_pass2<INV>(tw, k2, r));
    dft16<INV>(v);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 16; ++r) img[pad((j >> 4) * 256 + k2 + 16 * r)] = v[r];
    __builtin_amdgcn_wave_barrier();
    // pass 3: Ns = 256, radix 4; butterfly b of this lane: j' = j + 64 b, src[j' + 256 r],
    // twiddle W_1024^{j' r}, output index j' + 256 r  -> v[b + 4 r]
    cf o[16];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int jp = j + 64 * b;
        cf a0 = img[pad(jp)], a1 = img[pad(jp + 256)], a2 = img[pad(jp + 512)], a3 = img[pad(jp + 768)];
        a1 = cmulw(a1, tw_pass3<INV>(tw, jp, 1));
        a2 = cmulw(a2, tw_pass3<INV>(tw, jp, 2));
        a3 = cmulw(a3, tw_pass3<INV>(tw, jp, 3));
        dft4<INV>(a0, a1, a2, a3);
        o[b] = a0;
        o[b + 4] = a1;
        o[b + 8] = a2;
        o[b + 12] = a3;
    }
    __builtin_amdgcn_wave_barrier(); // the image is rewritten by this wave's next transform
#pragma unroll
    for (int m = 0; m < 16; ++m) v[m] = o[m];
}

// Frame f of a stream of nframes frames, lane j holding samples j + 64 m (nsh::fft::load16 / store16)
__device__ __forceinline__ void load_frame16(cf (&v)[16], const float2* __restrict__ in, int64_t f, int64_t nframes)
{
    nsh::fft::load16<N>(v, in, f, nframes * N, nsh::fft::lane64{ (int)(threadIdx.x & 63) });
}
__device__ __forceinline__ void store_frame16(const cf (&v)[16], float2* __restrict__ out, int64_t f, int64_t nframes)
{
    nsh::fft::store16<N>(v, out, f, nframes * N, nsh::fft::lane64{ (int)(threadIdx.x & 63) });
}

constexpr int FPW = NT / 64; // frames (waves) per workgroup

template <bool INV>
__global__ __launch_bounds__(NT) void k_fft1024(const float2* __restrict__ in, float2* __restrict__ out, int64_t nframes,
                                                const float2* __restrict__ tw_g)
{
    __shared__ cf tw[TWN];
    __shared__ cf img_all[FPW * WLDS];
    stage_twiddles(tw, tw_g, threadIdx.x, NT);
    __syncthreads();
    cf* img = img_all + (threadIdx.x >> 6) * WLDS;
    const int64_t stride = (int64_t)gridDim.x * FPW;
    int64_t f = (int64_t)blockIdx.x * FPW + (threadIdx.x >> 6);
    if (f >= nframes) return;
    cf v[16], nx[16];
    load_frame16(v, in, f, nframes);
    for (; f < nframes; f += stride) {
        load_frame16(nx, in, f + stride, nframes);
        fft_wave<INV>(v, img, tw);
        store_frame16(v, out, f, nframes);
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = nx[m];
    }
}

// No register prefetch of the next frame here (unlike k_fft1024): without it and with the
// weights in LDS the kernel fits 168 VGPRs, i.e. 3 workgroups (12 waves) per CU, and that
// occupancy hides the load latency better: 816 vs 858 us per 2^28 samples
// (tools/probe/fft_ab.py history in DESIGN.md section 4).
constexpr int CFPW = 4; // channelizer frames (waves) per workgroup
// the launch bounds' minimum workgroups per CU (2 lets the compiler take up to 256 VGPRs: 2 waves per SIMD)
constexpr int CHAN_MINWG = 2;
template <int FW>
__global__ __launch_bounds__(64 * FW, CHAN_MINWG) void k_chan1024(const float2* __restrict__ in, float2* __restrict__ out, int64_t nframes,
                                                    const float2* __restrict__ tw_g, const float2* __restrict__ w)
{
    __shared__ cf tw[TWN];
    __shared__ cf wl[N];
    __shared__ cf img_all[FW * WLDS];
    stage_twiddles(tw, tw_g, threadIdx.x, 64 * FW);
    for (int t = threadIdx.x; t < N; t += 64 * FW) wl[t] = cf{ w[t].x, w[t].y };
    __syncthreads();
    cf* img = img_all + (threadIdx.x >> 6) * WLDS;
    const int j = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * FW;
    cf v[16];
    for (int64_t f = (int64_t)blockIdx.x * FW + (threadIdx.x >> 6); f < nframes; f += stride) {
        load_frame16(v, in, f, nframes);
        fft_wave<false>(v, img, tw);
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = cmul_rn(v[m], wl[j + 64 * m]);
        fft_wave<true>(v, img, tw);
        store_frame16(v, out, f, nframes);
    }
}

std::mutex g_tw_mtx;
std::vector<float2*> g_tw(64, nullptr); // per device

int twiddles(int dev, const float2** tw)
{
    std::lock_guard<std::mutex> g(g_tw_mtx);
    if (dev < 0 || dev >= (int)g_tw.size()) return nsh::fail_msg("fft: bad device");
    if (!g_tw[dev]) {
        std::vector<float2> h(N);
        for (int t = 0; t < N; ++t) h[t] = nsh::fft::twiddle(t, N);
        float2* d = nullptr;
        NSH_CK(hipMalloc(&d, N * sizeof(float2)));
        NSH_CK(hipMemcpy(d, h.data(), N * sizeof(float2), hipMemcpyHostToDevice));
        g_tw[dev] = d;
    }
    *tw = g_tw[dev];
    return 0;
}

// Workgroups of the grid-stride walk over frames: enough that each walks only a few frame groups.
// With 4096 (16 groups each) the last long-running workgroups left CUs idle at the end of a 2^28
// launch: 16384 workgroups run the channelizer 5 % faster (806 -> 754-774 us, 66.5 -> 69.4-71.2 %),
// 24576 the fft1024 13 % faster (768 -> 670 us = 80 % of 8 TB/s); 65536 (one frame per wave, the
// tables staged per frame) is slower for both (r05zt, r05zu: both orders, bit-identical).
constexpr int FFT_CAP = 24576, CHAN_CAP = 16384;
} // namespace

extern "C" {

int nsh_fft1024_c2c(const float* in, float* out, int64_t nframes, int inverse, void* stream)
{
    nsh::launch_events_guard timing_guard; // an armed event pair never outlives this call
    if (nframes <= 0) return 0;
    if (!in || !out) return nsh::fail_msg("nsh_fft1024_c2c: null pointer");
    if (in == out) return nsh::fail_msg("nsh_fft1024_c2c: in-place not supported");
    return nsh::fft::fft1024_launch((const float2*)in, (float2*)out, nframes, inverse != 0, 0, nsh::S(stream), "nsh_fft1024_c2c");
}

int nsh_channelizer1024(const float* in, float* out, const float* w, int64_t nframes, void* stream)
{
    nsh::launch_events_guard timing_guard; // an armed event pair never outlives this call
    if (nframes <= 0) return 0;
    if (!in || !out || !w) return nsh::fail_msg("nsh_channelizer1024: null pointer");
    if (in == out) return nsh::fail_msg("nsh_channelizer1024: in-place not supported");
    int dev = 0;
    NSH_CK(hipGetDevice(&dev));
    const float2* tw = nullptr;
    if (int rc = twiddles(dev, &tw)) return rc;
    nsh::launch(k_chan1024<CFPW>, dim3(frame_grid(nframes, CFPW, CHAN_CAP)), dim3(64 * CFPW), 0, nsh::S(stream),
                       (const float2*)in, (float2*)out, nframes, tw, (const float2*)w);
    NSH_CK_LAUNCH("nsh_channelizer1024");
    return 0;
}

} // extern "C"

int nsh::fft::fft1024_launch(const float2* in, float2* out, int64_t nframes, bool inverse, int cap, hipStream_t s, const char* what)
{
    int dev = 0;
    NSH_CK(hipGetDevice(&dev));
    const float2* tw = nullptr;
    if (int rc = twiddles(dev, &tw)) return rc;
    const dim3 grid(frame_grid(nframes, FPW, cap > 0 ? cap : FFT_CAP));
    if (inverse)
        nsh::launch(k_fft1024<true>, grid, dim3(NT), 0, s, in, out, nframes, tw);
    else
        nsh::launch(k_fft1024<false>, grid, dim3(NT), 0, s, in, out, nframes, tw);
    NSH_CK_LAUNCH(what);
    return 0;
}
