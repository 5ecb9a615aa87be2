// What the two polyphase filterbank kernels share: k_pfb<M> (nsh_pfb.hip, analysis: branch FIRs, then
// the DFT) and k_pfb_synth<M> (nsh_pfb_synth.hip, synthesis: the DFT, then branch FIRs). The tile
// geometry and LDS images (described at k_pfb), the radix-2 lane-exchange DFT and its host twiddle
// table. tests/test_pfb_layout.py and tests/test_pfb_synth_layout.py restate them.
#pragma once
#include "nsh_stream_tile.hpp"

#include <cmath>

namespace nsh {
namespace pfb {

constexpr int kBlock = kStreamBlock;
constexpr int kR = 8;      // consecutive time steps a lane keeps
constexpr int kQC = 4;     // taps per chunk
constexpr int kRounds = 2; // store rounds: kR / kRounds time steps each

template <int M>
struct geom {
    static constexpr int LOG2M = ilog2(M);
    static constexpr int G = kBlock / M;    // time groups
    static constexpr int T = G * kR;        // time steps per workgroup
    static constexpr int RH = kR / kRounds; // time steps per store round
    static constexpr int YW = 64 * RH + 64; // entries of a wave's store image
    __host__ __device__ static constexpr int row_entry(int j) { return (M < 32 ? j + (j >> 3) : j) * M; }
    __host__ __device__ static constexpr int ypos(int e)
    {
        return M >= 32 ? e + (e >> 4) : e + ((e >> (ilog2(RH) + LOG2M)) << LOG2M);
    }
};

// Floats of the twiddle table of an M-point transform: max(log2 M - 1, 1) stages of M (cos, sin).
inline size_t twiddle_floats(int M) { return 2 * (size_t)std::max(ilog2(M) - 1, 1) * M; }

// tw[s M + lane] of stage s < log2 M - 1 (the last stage's twiddle is 1): 1 for the lane without the
// stage's bit, exp(+j 2 pi (lane mod half) / (2 half)) for the one with it; the quadrant points
// exactly, the rest from double. dst holds twiddle_floats(M) zeros.
inline void fill_twiddles(int M, float* dst)
{
    const int stages = ilog2(M);
    for (int s = 0; s < stages - 1; ++s) {
        const int half = M >> (s + 1);
        for (int q = 0; q < M; ++q) {
            double c = 1.0, sn = 0.0;
            if (q & half) {
                const int i = q & (half - 1);
                const double th = 2.0 * M_PI * (double)i / (double)(2 * half);
                c = std::cos(th), sn = std::sin(th);
                if (4 * i == 2 * half) c = 0.0, sn = 1.0;
            }
            dst[2 * ((size_t)s * M + q)] = (float)c;
            dst[2 * ((size_t)s * M + q) + 1] = (float)sn;
        }
    }
}

} // namespace pfb
} // namespace nsh
