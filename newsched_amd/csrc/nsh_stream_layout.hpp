// LDS layout choices of the one-launch stream kernels' plans (k_resamp, k_arb), host arithmetic
// only, no HIP: the plans (nsh_resamp.hip, nsh_arb.hip) and tests/cpp/qa_stream_layout.cpp, which
// prints the choices for the Python models of tests/ to compare, use this one copy.
//
// A ds_read_b64 serves lanes 0-31 and 32-63 separately, bank pair = entry mod 32; lanes that read
// the same entry are a broadcast. A layout's cost is the most different entries that any group of
// 32 lanes puts on one bank pair (1: conflict-free).
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>

namespace nsh {

constexpr int kStreamBlock = 256;    // threads of a stream kernel's workgroup
constexpr int kStreamMaxTile = 8192; // most samples of a tile's window (k_resamp with D > I, k_arb)

// The most different entries on one bank pair among n <= 32 entries.
inline int bank_pair_multiplicity(const int* entry, int n)
{
    int seen[32][32], count[32] = {}, worst = 0;
    for (int i = 0; i < n; ++i) {
        const int b = entry[i] & 31;
        bool dup = false;
        for (int k = 0; k < count[b]; ++k) dup = dup || seen[b][k] == entry[i];
        if (!dup) seen[b][count[b]++] = entry[i];
        worst = std::max(worst, count[b]);
    }
    return worst;
}

// The first candidate with the strictly smallest cost.
template <typename It, typename Cost>
inline int best_of(It first, It last, Cost cost)
{
    int best = *first, least = 1 << 30;
    for (; first != last; ++first) {
        const int m = cost(*first);
        if (m < least) least = m, best = *first;
    }
    return best;
}

// Shift padding, sample s at entry s + (s >> a): the candidates, 31 (none) first, so that a tie
// goes to the larger a, the smaller image.
constexpr int kShifts[] = { 31, 6, 5, 4, 3, 2, 1 };

// ---- k_resamp<R,P> ----------------------------------------------------------------------------
struct resamp_layout {
    int R;       // units per lane: the instantiation, by D / I
    bool linear; // k_resamp<8,1>: the packed image, a lane's units G apart
    int G;       // groups of R units per workgroup
    int a;       // the image's shift padding, 31: none
};

// Cost of shift a: over the lane groups of the workgroup and every window offset.
inline int resamp_worst_multiplicity(int I, int D, int R, int G, int a)
{
    int worst = 1;
    for (int c = 0; c < 64; ++c)
        for (int l0 = 0; l0 < kStreamBlock && l0 < G * I; l0 += 32) {
            int e[32], n = 0;
            for (int w = l0; w < l0 + 32 && w < G * I; ++w) {
                const int s = c + (w / I) * R * D + (w % I) * D / I;
                e[n++] = s + (s >> a);
            }
            worst = std::max(worst, bank_pair_multiplicity(e, n));
        }
    return worst;
}

inline resamp_layout resamp_layout_of(int I, int D)
{
    resamp_layout g;
    g.linear = D <= I;
    g.R = D <= 2 * I ? 8 : D <= 4 * I ? 4 : D <= 8 * I ? 2 : 1;
    g.G = std::max(1, std::min(kStreamBlock / I, kStreamMaxTile / (g.R * D)));
    g.a = g.linear ? 31 : best_of(std::begin(kShifts), std::end(kShifts), [&](int a) {
        return resamp_worst_multiplicity(I, D, g.R, g.G, a);
    });
    return g;
}

// ---- k_arb<R,P> -------------------------------------------------------------------------------
struct arb_layout {
    bool linear; // r >= 1: the packed sample image
    int a;       // the sample image's shift padding, 31: none
    int pad;     // tap k = j + q F at pair entry q (F + pad) + j + (j >> 5) pad
};

// Cost over 32 consecutive outputs at sampled phases: output l of the group is at c + l step,
// value(pos) is the entry it reads.
template <typename V>
inline int arb_worst_multiplicity(uint64_t step, int fshift, V value)
{
    int worst = 1;
    for (int ci = 0; ci < 64; ++ci)
        for (int cf = 0; cf < 4; ++cf) {
            // whole inputs and whole filter steps, and quarters of a step on top
            const uint64_t c = ((uint64_t)ci << (32 + fshift)) + (uint64_t)ci * 0x100000000ull + (uint64_t)cf * 0x40000000ull;
            int e[32];
            for (int l = 0; l < 32; ++l) e[l] = value(c + (uint64_t)l * step);
            worst = std::max(worst, bank_pair_multiplicity(e, 32));
        }
    return worst;
}

// step in Q32.32 filter steps per output, F = 2^fshift filters (nsh_arb_span.hpp)
inline arb_layout arb_layout_of(uint64_t step, int fshift)
{
    arb_layout g = { step <= 1ull << (32 + fshift), 31, 0 };
    if (!g.linear)
        g.a = best_of(std::begin(kShifts), std::end(kShifts), [&](int a) {
            return arb_worst_multiplicity(step, fshift, [&](uint64_t pos) {
                const int s = (int)(pos >> (32 + fshift));
                return s + (s >> a);
            });
        });
    if (fshift == 6) { // F = 64: j and j + 32 would share a bank pair
        int pads[32];
        std::iota(pads, pads + 32, 0);
        g.pad = best_of(pads, pads + 32, [&](int pad) {
            return arb_worst_multiplicity(step, fshift, [&](uint64_t pos) {
                const int j = (int)((pos >> 32) & 63);
                return j + (j >> 5) * pad;
            });
        });
    }
    return g;
}

} // namespace nsh
