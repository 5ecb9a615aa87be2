// Helpers of the FIR matrix-core kernels of nsh_fir_mfma.hip: k_fir_mfma12 / k_fir_exact12 for
// decim 1, k_fir_mfma13 / k_fir_exact13 (the default lockstep walk) and k_fir_mfma11 (the
// contiguous walk) for decim 2 / 4. The fp16x2 split, the range reduction, the fp32 direct form
// and the decimators' geometry, split stores, MFMA tile and output store -- one copy of each
// piece the kernels share -- plus two host helpers, in an anonymous namespace.
#pragma once
#include "nsh_common.hpp"
#include "nsh_fir_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>

namespace {


// CUs of the plan's device (queried once, at plan creation: a plan is read-only afterwards and
// may be shared by concurrent launches)
int plan_cus(const nsh_fir_plan* p) { return p->n_cu > 0 ? p->n_cu : 256; }

using nsh::buf_load_f4;
using nsh::buf_store_f2;
using nsh::chunk_rsrc;
using nsh::nf2;
using nsh::set_lds_attr;
using nsh::u32x2;
using nsh::virt;

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int TILE = 512;   // outputs per wave per chunk
constexpr int QMAX = 6;     // L <= 161


// ---- fp16x2: per-chunk scaled split, three products ------------------------------------------
// fp16 keeps 11 significant bits, so a two-term split x = x0 + x1 (both RNE) keeps 22 and
// three products x0h0 + x0h1 + x1h0 suffice (dropped x1h1 <= 2^-22 |xh|), where bf16 needs
// three terms and six products: half the matrix work. fp16's narrow
// exponent range is handled by power-of-two scaling, which is exact:
//  * taps: scaled once on the host so max |h| * 2^sh lies in [2^14, 2^15);
//  * samples: per 2048-sample chunk, 2^s with s from the largest magnitude in the chunk and
//    its halo (k_fir_mfma11: the chunk and its whole predecessor, which holds the halo), so
//    every scaled sample is < 2^15 (no fp16 overflow) and outputs are unscaled with one
//    power-of-two multiply or ldexp (exact unless subnormal).
// Per sample the split is then exact to 2^-22 relative, or 2^-39 of the chunk maximum for
// samples far below it (fp16 subnormal low term) -- below the fp32 direct form's own
// rounding error. A chunk holding a non-finite value, or a nonzero sample more than 2^28
// below the chunk maximum (its high term would be fp16-subnormal), takes an exact form
// instead: the exact-fp32 matrix tile (nsh_fir_f32_tile.hpp) if it is finite, else the fp32
// direct form (exact IEEE semantics, including inf/NaN). k_fir_mfma12 and k_fir_mfma13 queue
// such chunks for k_fir_exact12 / k_fir_exact13, launched right after them; k_fir_mfma11 filters
// them inline. Each wave writes its range of a chunk to an LDS slot and the workgroup agrees on
// the scale after a barrier; the scale differs between chunks, so a chunk's halo is split again
// from raw fp32 samples (loaded with the chunk, or k_fir_mfma11's LDS stash of the previous
// chunk's tail), not copied from the previous chunk's planes.
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
// A chunk's scale 2^sc applied to two adjacent samples' components (a register pair as loaded).
// MUL: one packed multiply by 2^sc, a normal float for sc in [-126, 127] -- a multiply by a power of
// two rounds exactly as ldexp does. scale_of gives sc >= -113 for finite chunks and up to 141 for
// chunks whose largest magnitude is below 2^-113: those (sc > 127) keep ldexp. The choice is
// workgroup-uniform: the kernels branch on scale_is_mul once per chunk, around all its split stores
// (as unscale_tile does on the output side).
__device__ __forceinline__ bool scale_is_mul(int sc) { return sc <= 127; }
template <bool MUL>
__device__ __forceinline__ nf2 scale2(float a, float b, int sc)
{
    if (MUL) return nf2{ a, b } * __builtin_bit_cast(float, (sc + 127) << 23);
    return nf2{ __builtin_ldexpf(a, sc), __builtin_ldexpf(b, sc) };
}
// fp16x2 split of the scaled pair (a, b): hi = RNE fp16 of each (one v_cvt_pk_f16_f32), lo = RNE
// fp16 of the exact residuals a - hi.a, b - hi.b. The residual has at most 13 significant bits, so
// it is exact in fp32 and fp16(fma(a, 1, -hi.a)) rounds once, to the same value as the subtract
// followed by a conversion: one v_fma_mix{lo,hi}_f16 per value, reading the fp32 sample and its
// half of the packed hi word, in place of two v_cvt_f32_f16, a v_pk_add_f32 and a
// v_cvt_pk_f16_f32 per pair. The compiler does not form it from C++ (it folds fma(-hi, 1, a) back
// to the subtract): inline asm.
__device__ __forceinline__ void split_pair16(float a, float b, unsigned& hi, unsigned& lo)
{
    const f16x2 h = __builtin_convertvector(f32x2{ a, b }, f16x2);
    hi = __builtin_bit_cast(unsigned, h);
    asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(lo) : "v"(a), "v"(hi));
    asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(lo) : "v"(b), "v"(hi));
}

// largest magnitude as a bit pattern: NaN-propagating v_maximum3_f32 with |.| operand modifiers
// (a NaN anywhere gives a NaN, i.e. bits >= 0x7f800000, as the integer form did)
__device__ __forceinline__ float max_abs(float a, float b) { return __builtin_elementwise_maximum(__builtin_fabsf(a), __builtin_fabsf(b)); }
__device__ __forceinline__ float max_abs4(const float4& v) { return __builtin_elementwise_maximum(max_abs(v.x, v.y), max_abs(v.z, v.w)); }
__device__ __forceinline__ unsigned max_mag(const float4& v) { return __float_as_uint(max_abs4(v)); }
// scale exponent: max magnitude (bit pattern) * 2^s in [2^14, 2^15) (zero/subnormal: 2^141)
__device__ __forceinline__ int scale_of(unsigned maxbits) { return 141 - (int)(maxbits >> 23); }
// Wave-wide max / min, uniform result: DPP within each 16-lane row (quad_perm xor 1, xor 2,
// row_ror 4, 8: VALU, no LDS) then the four row results by v_readlane. The __shfl_xor form
// was six dependent ds_bpermute round trips through the LDS unit per reduction.
template <bool MAX>
__device__ __forceinline__ unsigned wave_red(unsigned v)
{
    constexpr int id = MAX ? 0 : -1;
    auto op = [](unsigned a, unsigned b) { return MAX ? max(a, b) : min(a, b); };
    v = op(v, (unsigned)__builtin_amdgcn_update_dpp(id, (int)v, 0xB1, 0xf, 0xf, false));  // quad_perm [1,0,3,2]
    v = op(v, (unsigned)__builtin_amdgcn_update_dpp(id, (int)v, 0x4E, 0xf, 0xf, false));  // quad_perm [2,3,0,1]
    v = op(v, (unsigned)__builtin_amdgcn_update_dpp(id, (int)v, 0x124, 0xf, 0xf, false)); // row_ror:4
    v = op(v, (unsigned)__builtin_amdgcn_update_dpp(id, (int)v, 0x128, 0xf, 0xf, false)); // row_ror:8
    const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)v, 0), b = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
    const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)v, 32), d = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
    return op(op(a, b), op(c, d));
}
__device__ __forceinline__ unsigned wave_max(unsigned v) { return wave_red<true>(v); }
__device__ __forceinline__ unsigned wave_min(unsigned v) { return wave_red<false>(v); }
// min over components of (magnitude bits - 1): zero maps to 0xffffffff, so the chunk minimum
// is (smallest nonzero magnitude - 1), or ~0u for an all-zero chunk
// smallest nonzero magnitude, coded as 2 |x|_bits - 1 (one v_lshl_add per value; zero -> ~0u)
__device__ __forceinline__ unsigned nz_code(float x) { return (__float_as_uint(x) << 1) - 1u; }
__device__ __forceinline__ unsigned min_nz1(const float4& v)
{
    return min(min(nz_code(v.x), nz_code(v.y)), min(nz_code(v.z), nz_code(v.w)));
}
// The exact-path rule over a whole chunk: non-finite iff its largest magnitude is; a nonzero sample
// scales below fp16's normal range iff its smallest nonzero one does (ldexp is exact, monotonic)
__device__ __forceinline__ bool chunk_needs_exact(unsigned maxbits, unsigned mnz1, int s)
{
    if (maxbits >= 0x7f800000u) return true;
    if (mnz1 == ~0u) return false; // all zero
    return __builtin_ldexpf(__uint_as_float((mnz1 >> 1) + 1u), s) < 6.103515625e-05f; // 2^-14
}
// A wave's range over a chunk in registers: largest magnitude m (bit pattern) and smallest nonzero
// code z (min_nz1), starting from (mf, z0) -- the thread's halo samples', or (0.f, ~0u) for none
__device__ __forceinline__ void wave_range(const float4 (&v)[4], float mf, unsigned z0, unsigned& m, unsigned& z)
{
    z = z0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        mf = __builtin_elementwise_maximum(mf, max_abs4(v[u]));
        z = min(z, min_nz1(v[u]));
    }
    m = wave_max(__float_as_uint(mf));
    z = wave_min(z);
}
// The workgroup's range from its four waves' LDS slots
__device__ __forceinline__ unsigned slots_max(const unsigned* s) { return max(max(s[0], s[1]), max(s[2], s[3])); }
__device__ __forceinline__ unsigned slots_min(const unsigned* s) { return min(min(s[0], s[1]), min(s[2], s[3])); }

// chunk ch -> registers: lane t holds samples (2t, 2t+1) + 512 u, u < 4
__device__ __forceinline__ void load_chunk9(float4 (&v)[4], const float2* __restrict__ in, int64_t ch, int64_t n_in)
{
    const __amdgpu_buffer_rsrc_t r = chunk_rsrc<2048>(in, ch, n_in);
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = buf_load_f4(r, (threadIdx.x + 256 * u) * 16);
}

__device__ __forceinline__ float2 f4_sample(const float4& v, int which)
{
    return which ? make_float2(v.z, v.w) : make_float2(v.x, v.y);
}

// The exact path on a raw fp32 chunk in LDS (local sample j at float2 index j, halo first):
// the lane's 8 outputs by the fp32 direct form (taps in order, fused multiply-add per component).
// The 8 outputs are two groups of four, 32 samples apart (blocks (reg & 3) + 8 (reg >> 2) + 4 h):
// an input sample j0 + q feeds output b of its group through tap k = 32 b - q, so each sample is
// read from LDS once per group (L + 96 reads instead of 4 L). q = 32 c - r runs downward, so every
// output still takes its taps in the order k = 0, 1, ..., L - 1 (bit-identical to one output at a
// time). (c, r, b) are unrolled, so every tap index k = 32 (b - c) + r is a compile-time constant:
// the tap loads are unconditional scalar loads the compiler batches ahead of use, and only taps of
// the last 32-block (k > 32 (Q - 2); Q = (L + 30) / 32 + 1 makes every earlier k < L) test k < L.
// re and im go through one v_pk_fma_f32.
// The same input reuse for NG outputs SP raw samples apart (output b at raw[j0 + SP b]): taps of
// index k > HMAX are zero (L - 1 <= HMAX), and every k <= KSAFE is below L.
template <int NG, int SP, int HMAX, int KSAFE>
__device__ __forceinline__ void direct_group(const nf2* raw, int j0, const float* __restrict__ taps, int L, nf2 (&acc)[NG])
{
#pragma unroll
    for (int b = 0; b < NG; ++b) acc[b] = nf2{ 0.f, 0.f };
#pragma unroll
    for (int i = 0; i <= SP * (NG - 1) + HMAX; ++i) {
        const int q = SP * (NG - 1) - i;
        const nf2 x = raw[j0 + q];
#pragma unroll
        for (int b = 0; b < NG; ++b) {
            const int k = SP * b - q;
            if (k < 0 || k > HMAX) continue;
            const float t = taps[k < L ? k : L - 1];
            if (k > KSAFE && k >= L) continue;
            acc[b] = __builtin_elementwise_fma(nf2{ t, t }, x, acc[b]);
        }
    }
}

template <int Q>
__device__ __forceinline__ void direct_tile9(const unsigned char* lds, const float* __restrict__ taps, int L, int wave, int h,
                                             int phase, nf2 (&o)[8])
{
    constexpr int H = 32 * (Q - 1); // halo samples (geom12)
    const nf2* raw = reinterpret_cast<const nf2*>(lds);
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int j0 = H + wave * TILE + 32 * (8 * g + 4 * h) + phase;
        nf2 acc[4] = { nf2{ 0.f, 0.f }, nf2{ 0.f, 0.f }, nf2{ 0.f, 0.f }, nf2{ 0.f, 0.f } };
#pragma unroll
        for (int c = 3; c >= -(Q - 1); --c) {
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                const int q = 32 * c - r;
                if (q < -H) break;  // L - 1 <= H: no tap reaches further back
                const nf2 x = raw[j0 + q];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int k = 32 * (b - c) + r;
                    if (k < 0 || k > H) continue;
                    const float t = taps[k < L ? k : L - 1];
                    if (k > 32 * (Q - 2) && k >= L) continue;
                    acc[b] = __builtin_elementwise_fma(nf2{ t, t }, x, acc[b]);
                }
            }
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) o[4 * g + b] = acc[b];
    }
}

// ---- k_fir_mfma13 / k_fir_mfma11: decimating polyphase FIR (D = 2, 4) on the fp16x2 split ----
// The polyphase Toeplitz form (phase streams z_0[i] = x[D i], z_r[i] = x[D i + D - r], taps
// h'_0[j] = h[D j], h'_r[j] = h[D (j - 1) + r], 16-sample blocks, 16x16x32 + 16x16x16 tail): two
// fp16 planes per component and three products, per-chunk power-of-two scale, buffer
// loads/stores, LDS-only barriers. The halo (the D*H input samples before the chunk) is kept raw
// in an LDS stash and split at each chunk's scale. What the two walks share is below; the walks
// themselves and the exact forms are in nsh_fir_mfma.hip.
// k_fir_mfma13 (CLOAD): each chunk-load instruction reads 1 KiB contiguous (nontemporal), lane pairs
// exchange their samples by DPP before the split stores; k_fir_mfma11 keeps a thread's D float4 side
// by side (each instruction spread over D KiB). On k_fir_mfma13 at D = 4, bit-identical: faster on
// three boxes of four (72.5 vs 70.1 %, r05ze; ~1 % in four two-library A/Bs each on two more, r05zzd),
// 1.3 % slower on one (r05zg)
template <int D, int QH>
struct geom11 {
    static constexpr int NT = 256;
    static constexpr int CHUNK_IN = 2048;
    static constexpr int CHUNK = CHUNK_IN / D;
    static constexpr int TILES = 4 / D;
    static constexpr int WAVE_OUT = TILES * 128;
    static constexpr int KS = QH / 2;
    static constexpr int TAIL = QH % 2;
    static constexpr int H = 16 * (QH - 1);                    // halo samples per phase
    static constexpr int HR = QH - 1;
    static constexpr int NB = (CHUNK + H) / 16;
    static constexpr int PLANE = NB * 32;
    static constexpr int IM_OFF = (2 * PLANE + 255) / 256 * 256 + 128;
    // phase planes PH apart; k_fir_mfma13's split stores (CLOAD) write all D phases in one
    // instruction, 32 / D pairs each per 32-lane group: PH = 32 * (4 / D) mod 128 B puts them on
    // disjoint banks
    static constexpr int PH = (IM_OFF + 2 * PLANE + 255) / 256 * 256 + 128 / D;
    static constexpr int BUF = (D * PH + 255) / 256 * 256;
    static constexpr int HP = D * H / 2;                      // halo float4 (2 input samples each)
    static constexpr int STASH = HP * 16;
    static constexpr int SLOTS = 2 * BUF + 2 * STASH;
    static constexpr int LDS = SLOTS + 64;                     // u32 max[2][4], mnz[2][4]
    static constexpr int UNITS = 4 / D;                        // units of 2D samples per thread
    static constexpr int PER_PHASE = 2 * KS * 64 * 8 + 2 * 64 * 4; // fp16 tap elements
    static_assert(D == 2 || D == 4, "D");
    static_assert((HP + 1024) * 16 <= BUF, "a raw fp32 chunk + halo fits one plane buffer");
    static_assert(HP <= NT && H / 2 <= NT, "halo: one float4 per thread");
};

// the pair of scaled samples a, b (time s, s + 1 of phase r) -> the phase's four planes
template <class G>
__device__ __forceinline__ void store_pair_g(unsigned char* buf, int r, int s, nf2 a, nf2 b)
{
    unsigned char* ph = buf + r * G::PH;
    const int off = (s >> 4) * 32 + (s & 15) * 2;
    unsigned rh, rl, ih, il;
    split_pair16(a.x, b.x, rh, rl);
    split_pair16(a.y, b.y, ih, il);
    *reinterpret_cast<unsigned*>(ph + off) = rh;
    *reinterpret_cast<unsigned*>(ph + G::PLANE + off) = rl;
    *reinterpret_cast<unsigned*>(ph + G::IM_OFF + off) = ih;
    *reinterpret_cast<unsigned*>(ph + G::IM_OFF + G::PLANE + off) = il;
}
// o = s * 2^u per (re, im) pair: one packed multiply when 2^u is a normal float (it rounds as
// ldexp does), else ldexp
template <int M>
__device__ __forceinline__ void unscale_tile(const nf2 (&s)[M], int u, nf2 (&o)[M])
{
    if (u >= -126 && u <= 127) {
        const float f = __builtin_bit_cast(float, (u + 127) << 23);
#pragma unroll
        for (int i = 0; i < M; ++i) o[i] = s[i] * f;
    } else {
#pragma unroll
        for (int i = 0; i < M; ++i) o[i] = nf2{ __builtin_ldexpf(s[i].x, u), __builtin_ldexpf(s[i].y, u) };
    }
}
template <int D, int QH>
__device__ __forceinline__ void store_pair11(unsigned char* buf, int r, int s, nf2 a, nf2 b)
{
    store_pair_g<geom11<D, QH>>(buf, r, s, a, b);
}

// the chunk's float4 (2 input samples) a lane loads as its unit u, instruction f, with
// CLOAD: the wave's 64 D float4 of unit u in D contiguous 1 KiB runs
template <int D>
__device__ __forceinline__ int q13(int u, int f)
{
    return 64 * D * ((int)(threadIdx.x >> 6) + 4 * u) + 64 * f + (int)(threadIdx.x & 63);
}

// chunk (registers) + its raw halo (hsrc: HP float4 in LDS) -> the split phase planes at scale 2^sc.
// CLOAD: v[u D + f] is the chunk's float4 q13(u, f) (k_fir_mfma13's whole-line loads), else float4
// (tid + NT u) D + f (a thread's D float4 adjacent). Every sample is scaled as loaded (a packed
// multiply per (re, im) register pair, MUL: scale2), before the lanes exchange and split them.
template <int D, int QH, bool CLOAD, bool MUL>
__device__ __forceinline__ void put_split11_as(int tid, unsigned char* buf, const float4* hsrc, const float4 (&v)[4], int sc)
{
    using G = geom11<D, QH>;
    if (tid < D * (G::H / 2)) { // halo: phase r, pair pi from the raw halo samples
        const int r = tid / (G::H / 2), pi = tid % (G::H / 2);
        const int sr = r == 0 ? 0 : D - r;
        const int pa = D * (2 * pi) + sr, pb = D * (2 * pi + 1) + sr;
        const float2 a = f4_sample(hsrc[pa >> 1], pa & 1), bb = f4_sample(hsrc[pb >> 1], pb & 1);
        store_pair11<D, QH>(buf, r, 2 * pi, scale2<MUL>(a.x, a.y, sc), scale2<MUL>(bb.x, bb.y, sc));
    }
    if constexpr (CLOAD) {
        // float4 q holds samples 2q, 2q + 1: phase offsets 2q mod D (+1) at time 2q / D, the pair
        // 2q / 2D, its time bit k = q & (D / 2). Lanes q and q ^ (D / 2) hold the same offsets at the
        // pair's two times: each keeps offset k and takes the partner's (one DPP exchange per float),
        // then stores one phase pair -- all D phases in each store instruction (PH padded for it)
        constexpr int XCHG = D == 4 ? 0x4e : 0xb1; // quad_perm [2,3,0,1] / [1,0,3,2]: lane ^ (D / 2)
#pragma unroll
        for (int u = 0; u < G::UNITS; ++u)
#pragma unroll
            for (int f = 0; f < D; ++f) {
                const int q = q13<D>(u, f);
                const bool k = (q & (D / 2)) != 0;
                const nf2 x0 = scale2<MUL>(v[u * D + f].x, v[u * D + f].y, sc), x1 = scale2<MUL>(v[u * D + f].z, v[u * D + f].w, sc);
                const float kre = k ? x1.x : x0.x, kim = k ? x1.y : x0.y; // offset k: kept
                const float sre = k ? x0.x : x1.x, sim = k ? x0.y : x1.y; // offset 1 - k: the partner's
                const float rre = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(sre), XCHG, 0xf, 0xf, true));
                const float rim = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(sim), XCHG, 0xf, 0xf, true));
                const int sr = D == 4 ? 2 * (q & 1) + (int)k : (int)k;
                const int r = sr == 0 ? 0 : D - sr;
                const int s = G::H + 2 * (q / D);
                // the pair in time order, by selects: a per-lane branch around the split's inline asm
                // would stay a branch (both sides executed, lanes masked)
                store_pair11<D, QH>(buf, r, s, nf2{ k ? rre : kre, k ? rim : kim }, nf2{ k ? kre : rre, k ? kim : rim });
            }
    } else {
#pragma unroll
        for (int u = 0; u < G::UNITS; ++u) {
            const int i0 = 2 * (tid + G::NT * u);
#pragma unroll
            for (int r = 0; r < D; ++r) {
                const int sr = r == 0 ? 0 : D - r;
                const int la = sr, lb = D + sr;
                const float2 a = f4_sample(v[u * D + la / 2], la & 1);
                const float2 bb = f4_sample(v[u * D + lb / 2], lb & 1);
                store_pair11<D, QH>(buf, r, G::H + i0, scale2<MUL>(a.x, a.y, sc), scale2<MUL>(bb.x, bb.y, sc));
            }
        }
    }
}
// the form of the scale (workgroup-uniform) chosen once for the chunk
template <int D, int QH, bool CLOAD>
__device__ __forceinline__ void put_split11(int tid, unsigned char* buf, const float4* hsrc, const float4 (&v)[4], int sc)
{
    if (__builtin_expect(scale_is_mul(sc), 1))
        put_split11_as<D, QH, CLOAD, true>(tid, buf, hsrc, v, sc);
    else
        put_split11_as<D, QH, CLOAD, false>(tid, buf, hsrc, v, sc);
}

// A lane's place in the decimators' tile: component c and block b of its A row (row_base: byte
// offset of that row in a phase's planes), k-group g, output phase
template <int D, int QH>
struct lane11 {
    using G = geom11<D, QH>;
    const int lane, wave, g, phase, row_base;
    __device__ __forceinline__ explicit lane11(int tid)
        : lane(tid & 63), wave(tid >> 6), g(lane >> 4), phase(lane & 15),
          row_base((lane & 1) * G::IM_OFF + (G::HR + wave * (G::WAVE_OUT / 16) + ((lane & 15) >> 1)) * 32)
    {
    }
};

// The split MFMA tile: the wave's WAVE_OUT outputs of the chunk staged at cur, D phases x (KS
// k-steps of 32 + a 16-wide tail for odd QH) x three products, from the lane's tap fragments
// (B0 / T0: hi, B1 / T1: lo), unscaled by 2^unscale. k_fir_mfma13 keeps an open-coded copy (see
// there): change both together.
template <int D, int QH>
__device__ __forceinline__ void mfma_tile11(const unsigned char* cur, const lane11<D, QH>& ln,
                                            const f16x8 (&B0)[D][geom11<D, QH>::KS + 1], const f16x8 (&B1)[D][geom11<D, QH>::KS + 1],
                                            const f16x4 (&T0)[D], const f16x4 (&T1)[D], int unscale,
                                            nf2 (&o)[2 * geom11<D, QH>::TILES])
{
    using G = geom11<D, QH>;
    constexpr int KS = G::KS;
    const int g = ln.g, row_base = ln.row_base;
    f32x4 hi[G::TILES], lo[G::TILES], hi_t[G::TILES], lo_t[G::TILES];
#pragma unroll
    for (int t = 0; t < G::TILES; ++t) {
        hi[t] = f32x4{ 0.f, 0.f, 0.f, 0.f };
        lo[t] = f32x4{ 0.f, 0.f, 0.f, 0.f };
        hi_t[t] = f32x4{ 0.f, 0.f, 0.f, 0.f };
        lo_t[t] = f32x4{ 0.f, 0.f, 0.f, 0.f };
    }
#pragma unroll
    for (int r = 0; r < D; ++r) {
        const unsigned char* ph = cur + r * G::PH;
#pragma unroll
        for (int st = 0; st < KS; ++st) {
            const int q = 2 * st + (g >> 1);
#pragma unroll
            for (int t = 0; t < G::TILES; ++t) {
                const int off = row_base + t * 8 * 32 - q * 32 + (g & 1) * 16;
                const f16x8 A0 = *reinterpret_cast<const f16x8*>(ph + off);
                const f16x8 A1 = *reinterpret_cast<const f16x8*>(ph + off + G::PLANE);
                hi[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A0, B0[r][st], hi[t], 0, 0, 0);
                lo[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A0, B1[r][st], lo[t], 0, 0, 0);
                lo[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A1, B0[r][st], lo[t], 0, 0, 0);
            }
        }
        if constexpr (G::TAIL) { // separate accumulators: see v5_compute
            // single ds_read_b64 (the empty asm keeps the compiler from pairing the tiles'
            // reads into ds_read2_b64, whose 16-lane groups see the re and im rows 4 apart on
            // one bank: 4-way, 43-50 % of the kernel's LDS cycles in profiles/r03o_pmc_decim.json;
            // as ds_read_b64, 2-way)
#pragma unroll
            for (int t = 0; t < G::TILES; ++t) {
                const int off = row_base + t * 8 * 32 - (QH - 1) * 32 + g * 8;
                const f16x4 A0 = *reinterpret_cast<const f16x4*>(ph + off);
                asm volatile("" ::: "memory");
                const f16x4 A1 = *reinterpret_cast<const f16x4*>(ph + off + G::PLANE);
                asm volatile("" ::: "memory");
                hi_t[t] = __builtin_amdgcn_mfma_f32_16x16x16f16(A0, T0[r], hi_t[t], 0, 0, 0);
                lo_t[t] = __builtin_amdgcn_mfma_f32_16x16x16f16(A0, T1[r], lo_t[t], 0, 0, 0);
                lo_t[t] = __builtin_amdgcn_mfma_f32_16x16x16f16(A1, T0[r], lo_t[t], 0, 0, 0);
            }
        }
    }
    nf2 sum[2 * G::TILES];
#pragma unroll
    for (int t = 0; t < G::TILES; ++t)
#pragma unroll
        for (int half = 0; half < 2; ++half)
            sum[2 * t + half] = (nf2{ hi[t][2 * half], hi[t][2 * half + 1] } + nf2{ hi_t[t][2 * half], hi_t[t][2 * half + 1] }) +
                                (nf2{ lo[t][2 * half], lo[t][2 * half + 1] } + nf2{ lo_t[t][2 * half], lo_t[t][2 * half + 1] });
    unscale_tile(sum, unscale, o);
}

// The decimators' output store: o[oi] is output wave WAVE_OUT + 16 (8 (oi >> 1) + 2 g + (oi & 1)) + phase
// of chunk ch
template <int D, int QH>
__device__ __forceinline__ void store_tile11(float2* __restrict__ out, int64_t ch, int64_t n_out, const lane11<D, QH>& ln,
                                             const nf2 (&o)[2 * geom11<D, QH>::TILES])
{
    using G = geom11<D, QH>;
    const __amdgpu_buffer_rsrc_t r = chunk_rsrc<G::CHUNK>(out, ch, n_out);
#pragma unroll
    for (int oi = 0; oi < 2 * G::TILES; ++oi)
        buf_store_f2(r, (ln.wave * G::WAVE_OUT + ((oi >> 1) * 8 + 2 * ln.g + (oi & 1)) * 16 + ln.phase) * 8, o[oi]);
}

// Host: the taps' scale exponent sh (max |h| * 2^sh in [2^14, 2^15), scale_of on the host) and the
// fp16 hi / lo split (RNE) of one scaled tap
int tap_scale(const nsh_fir_plan* p)
{
    unsigned maxbits = 0;
    for (float t : p->taps_host) {
        unsigned u;
        std::memcpy(&u, &t, 4);
        maxbits = std::max(maxbits, u & 0x7fffffffu);
    }
    return 141 - (int)(maxbits >> 23);
}
void split_tap(float h, int sh, _Float16& hi, _Float16& lo)
{
    const float hs = std::ldexp(h, sh);
    hi = (_Float16)hs;
    lo = (_Float16)(hs - (float)hi);
}


int decim_qh(const nsh_fir_plan* p) { return ((p->L + p->D - 1) / p->D + 1 + 15 + 15) / 16; }
bool finite_taps(const nsh_fir_plan* p)
{
    for (float t : p->taps_host)
        if (!(t == t) || t - t != 0.f) return false;
    return true;
}

} // namespace
