// The 64-bit phase's phasor, shared by the rotating kernels (k_rotate and k_fir_xlat in
// nsh_xlat.hip, k_fft_xlat in nsh_fft_xlat_kernel.hpp); nsh_xlat.hip's header comment has the phase's
// definition. gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace nsh {

// exp(j 2 pi p / 2^64) from the top 32 bits of p
__device__ __forceinline__ float2 phasor(uint64_t p)
{
    const int s = (int)(uint32_t)(p >> 32);
    float sn, cs;
    sincospif((float)s * 4.656612873077392578125e-10f /* 2^-31 */, &sn, &cs);
    return make_float2(cs, sn);
}
// a * w, complex; one rounded product and one FMA per component
__device__ __forceinline__ float2 crot(float2 a, float2 w)
{
    return make_float2(__builtin_fmaf(-a.y, w.y, a.x * w.x), __builtin_fmaf(a.x, w.y, a.y * w.x));
}

} // namespace nsh
