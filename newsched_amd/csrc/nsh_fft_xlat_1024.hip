// libnsh_hip.so: the seven decimations of k_fft_xlat<1024, D> and the form without rotation
// (nsh_fft_xlat_kernel.hpp); a file per frame size, so that the 32 forms build side by side.
#include "nsh_fft_xlat_kernel.hpp"

NSH_FFT_XLAT_FORMS(1024)
