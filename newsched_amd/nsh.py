"""ctypes binding of libnsh_hip.so (include/nsh_hip.h) -- the MI355X kernel shim.

This module is the Python view of the C-ABI boundary; the C++17 newsched host links the
same library directly. It never falls back to a CPU implementation: if the in-tree
library is missing, `lib()` raises.

Device memory and streams on the Python side are torch tensors / torch streams (plumbing
only); every pointer handed to the shim is a raw device address.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")
HIP_LIB = os.path.join(LIB_DIR, "libnsh_hip.so")
# NSH_HIP_LIB: another build of the library (A/B probes)
HIP_LIB = os.environ.get("NSH_HIP_LIB") or HIP_LIB

NSH_H2D, NSH_D2H, NSH_D2D, NSH_DEFAULT = 0, 1, 2, 3
FIR_AUTO, FIR_DIRECT, FIR_MFMA, FIR_MFMA16, FIR_MFMA_BF16X3, FIR_MFMA_F32, FIR_PFFT = 0, 1, 2, 3, 4, 5, 6

# name -> (restype, argtypes); mirrors include/nsh_hip.h exactly (tests check the header).
_vp, _i, _i64, _u64, _sz, _f = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_size_t, C.c_float
SIGNATURES = {
    "nsh_abi_version": (_i, []),
    "nsh_last_error": (C.c_char_p, []),
    "nsh_get_device_count": (_i, [C.POINTER(_i)]),
    "nsh_set_device": (_i, [_i]),
    "nsh_device_info": (_i, [_i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_sz), C.c_char_p, _i]),
    "nsh_device_pci_id": (_i, [_i, C.c_char_p, _i]),
    "nsh_pointer_device": (_i, [_vp, C.POINTER(_i)]),
    "nsh_device_sync": (_i, []),
    "nsh_stream_create": (_i, [_i, C.POINTER(_vp)]),
    "nsh_stream_destroy": (_i, [_vp]),
    "nsh_stream_sync": (_i, [_vp]),
    "nsh_stream_query": (_i, [_vp]),
    "nsh_event_create": (_i, [C.POINTER(_vp)]),
    "nsh_event_destroy": (_i, [_vp]),
    "nsh_event_record": (_i, [_vp, _vp]),
    "nsh_event_query": (_i, [_vp]),
    "nsh_event_sync": (_i, [_vp]),
    "nsh_event_elapsed_ms": (_i, [_vp, _vp, C.POINTER(_f)]),
    "nsh_stream_wait_event": (_i, [_vp, _vp]),
    "nsh_time_next_launch": (_i, [_vp, _vp]),
    "nsh_timed_launches": (_i, [C.POINTER(_u64)]),
    "nsh_clock_sample": (_i, [_vp, _i64, _vp]),
    "nsh_malloc": (_i, [_i, _sz, C.POINTER(_vp)]),
    "nsh_free": (_i, [_vp]),
    "nsh_host_alloc": (_i, [_sz, C.POINTER(_vp)]),
    "nsh_host_free": (_i, [_vp]),
    "nsh_memcpy_async": (_i, [_vp, _vp, _sz, _i, _vp]),
    "nsh_memset_async": (_i, [_vp, _i, _sz, _vp]),
    "nsh_ring_alloc": (_i, [_i, _sz, C.POINTER(_vp), C.POINTER(_sz), C.POINTER(_i)]),
    "nsh_ring_free": (_i, [_vp]),
    "nsh_ipc_mem_export": (_i, [_vp, _vp]),
    "nsh_ipc_mem_open": (_i, [_i, _vp, C.POINTER(_vp)]),
    "nsh_ipc_mem_close": (_i, [_vp]),
    "nsh_copy": (_i, [_vp, _vp, _sz, _vp]),
    "nsh_mul_const_cc": (_i, [_vp, _vp, _i64, _f, _f, _vp]),
    "nsh_mul_const_ff": (_i, [_vp, _vp, _i64, _f, _vp]),
    "nsh_mul_const_chain_cc": (_i, [_vp, _vp, _i64, C.POINTER(_f), _i, _vp]),
    "nsh_add_cc": (_i, [_vp, _vp, _vp, _i64, _vp]),
    "nsh_mul_cc": (_i, [_vp, _vp, _vp, _i64, _vp]),
    "nsh_mul_const_vcc": (_i, [_vp, _vp, _vp, _i, _i64, _vp]),
    "nsh_synth_cf32": (_i, [_vp, _i64, _u64, _u64, _vp]),
    "nsh_fir_plan_create": (_i, [_i, C.POINTER(_f), _i, _i, _i, C.POINTER(_vp)]),
    "nsh_fir_plan_destroy": (_i, [_vp]),
    "nsh_fir_plan_algo": (_i, [_vp]),
    "nsh_fir_plan_kernel": (C.c_char_p, [_vp]),
    "nsh_fir_ccf": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "nsh_fir_cascade_plan_create": (_i, [_i, C.POINTER(C.POINTER(_f)), C.POINTER(_i), C.POINTER(_i), _i,
                                         C.POINTER(_vp)]),
    "nsh_fir_cascade_plan_destroy": (_i, [_vp]),
    "nsh_fir_cascade_decim": (_i, [_vp]),
    "nsh_fir_cascade_hist_len": (_i, [_vp]),
    "nsh_fir_cascade_kernel": (C.c_char_p, [_vp]),
    "nsh_fir_cascade_ccf": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "nsh_phase_inc": (_i, [C.c_double, C.POINTER(_u64)]),
    "nsh_rotate_cc": (_i, [_vp, _vp, _i64, _u64, _u64, _vp]),
    "nsh_fir_xlat_plan_create": (_i, [_i, C.POINTER(_f), _i, _i, C.c_double, C.POINTER(_vp)]),
    "nsh_fir_xlat_plan_destroy": (_i, [_vp]),
    "nsh_fir_xlat_phase_inc": (_i, [_vp, C.POINTER(_u64)]),
    "nsh_fir_xlat_tile": (_i, [_vp]),
    "nsh_fir_xlat_kernel": (C.c_char_p, [_vp]),
    "nsh_fir_xlat_ccf": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _u64, _vp]),
    "nsh_pfb_plan_create": (_i, [_i, C.POINTER(_f), _i, _i, C.POINTER(_vp)]),
    "nsh_pfb_plan_destroy": (_i, [_vp]),
    "nsh_pfb_tile": (_i, [_vp]),
    "nsh_pfb_kernel": (C.c_char_p, [_vp]),
    "nsh_pfb_channelizer_ccf": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "nsh_pfb_synth_plan_create": (_i, [_i, C.POINTER(_f), _i, _i, C.POINTER(_vp)]),
    "nsh_pfb_synth_plan_destroy": (_i, [_vp]),
    "nsh_pfb_synth_tile": (_i, [_vp]),
    "nsh_pfb_synth_kernel": (C.c_char_p, [_vp]),
    "nsh_pfb_synthesizer_ccf": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "nsh_resamp_plan_create": (_i, [_i, C.POINTER(_f), _i, _i, _i, C.POINTER(_vp)]),
    "nsh_resamp_plan_destroy": (_i, [_vp]),
    "nsh_resamp_tile": (_i, [_vp]),
    "nsh_resamp_kernel": (C.c_char_p, [_vp]),
    "nsh_resamp_history": (_i, [_vp]),
    "nsh_resamp_ccf": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "nsh_arb_step": (_i, [C.c_double, _i, C.POINTER(_u64)]),
    "nsh_arb_span": (_i, [_u64, _i, _u64, _i64, _i64, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_u64)]),
    "nsh_arb_plan_create": (_i, [_i, C.POINTER(_f), _i, _i, C.c_double, C.POINTER(_vp)]),
    "nsh_arb_plan_destroy": (_i, [_vp]),
    "nsh_arb_tile": (_i, [_vp]),
    "nsh_arb_kernel": (C.c_char_p, [_vp]),
    "nsh_arb_history": (_i, [_vp]),
    "nsh_arb_plan_step": (_i, [_vp, C.POINTER(_u64)]),
    "nsh_arb_resamp_ccf": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _u64, _vp]),
    "nsh_fft1024_c2c": (_i, [_vp, _vp, _i64, _i, _vp]),
    "nsh_channelizer1024": (_i, [_vp, _vp, _vp, _i64, _vp]),
    "nsh_fft_plan_create": (_i, [_i, _i, _i, C.POINTER(_f), _i, C.POINTER(_vp)]),
    "nsh_fft_plan_destroy": (_i, [_vp]),
    "nsh_fft_plan_size": (_i, [_vp]),
    "nsh_fft_tile": (_i, [_vp]),
    "nsh_fft_kernel": (C.c_char_p, [_vp]),
    "nsh_fft_plan_grid_cap": (_i, [_vp, _i]),
    "nsh_fft_c2c": (_i, [_vp, _vp, _vp, _i64, _vp]),
    "nsh_fft_filter_plan_create": (_i, [_i, C.POINTER(_f), _i, _i, C.POINTER(_vp)]),
    "nsh_fft_filter_plan_destroy": (_i, [_vp]),
    "nsh_fft_filter_fft_size": (_i, [_vp]),
    "nsh_fft_filter_valid": (_i, [_vp]),
    "nsh_fft_filter_history": (_i, [_vp]),
    "nsh_fft_filter_tile": (_i, [_vp]),
    "nsh_fft_filter_kernel": (C.c_char_p, [_vp]),
    "nsh_fft_filter_grid_cap": (_i, [_vp, _i]),
    "nsh_fft_filter_ccc": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "nsh_fft_xlat_plan_create": (_i, [_i, C.POINTER(_f), _i, _i, C.c_double, _i, C.POINTER(_vp)]),
    "nsh_fft_xlat_plan_destroy": (_i, [_vp]),
    "nsh_fft_xlat_fft_size": (_i, [_vp]),
    "nsh_fft_xlat_decim": (_i, [_vp]),
    "nsh_fft_xlat_overlap": (_i, [_vp]),
    "nsh_fft_xlat_valid": (_i, [_vp]),
    "nsh_fft_xlat_history": (_i, [_vp]),
    "nsh_fft_xlat_phase_inc": (_i, [_vp, C.POINTER(_u64)]),
    "nsh_fft_xlat_tile": (_i, [_vp]),
    "nsh_fft_xlat_kernel": (C.c_char_p, [_vp]),
    "nsh_fft_xlat_grid_cap": (_i, [_vp, _i]),
    "nsh_fft_xlat_ccc": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _u64, _vp]),
    "nsh_psd_plan_create": (_i, [_i, _i, _i, C.POINTER(_f), _i, _f, _i, C.POINTER(_vp)]),
    "nsh_psd_plan_destroy": (_i, [_vp]),
    "nsh_psd_fft_size": (_i, [_vp]),
    "nsh_psd_navg": (_i, [_vp]),
    "nsh_psd_segment": (_i, [_vp]),
    "nsh_psd_tile": (_i, [_vp]),
    "nsh_psd_kernel": (C.c_char_p, [_vp]),
    "nsh_psd_grid_cap": (_i, [_vp, _i]),
    "nsh_psd_cf": (_i, [_vp, _vp, _vp, _i64, _vp]),
}

_lib = None
_lock = threading.Lock()


class NshError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load the in-tree libnsh_hip.so (raises if it was not built -- no fallback)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(HIP_LIB):
                raise NshError(f"{HIP_LIB} is missing: run `make hip` (or __graft_entry__.build())")
            L = C.CDLL(HIP_LIB, mode=C.RTLD_GLOBAL)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            _lib = L
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().nsh_last_error().decode(errors="replace")
        raise NshError(f"{what or 'nsh call'} failed (rc={rc}): {msg}")


def ptr(t) -> int:
    """Raw device address of a torch tensor (or an int passthrough)."""
    return t if isinstance(t, int) else t.data_ptr()


def _opt_ptr(t):
    """ptr(t), or None (a NULL pointer) for None."""
    return None if t is None else ptr(t)


def stream_ptr(stream=None) -> int:
    import torch

    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream


def pointer_device(p) -> int:
    """The GPU whose device memory p points into, -1 for host memory / NULL (nsh_pointer_device)."""
    d = C.c_int(-2)
    check(lib().nsh_pointer_device(C.c_void_p(ptr(p)), C.byref(d)), "nsh_pointer_device")
    return d.value


# ---- thin typed wrappers over torch tensors (complex64 or float32 views) -------------
def copy(src, dst, nbytes: int, stream=None):
    check(lib().nsh_copy(ptr(src), ptr(dst), nbytes, stream_ptr(stream)), "nsh_copy")


def mul_const_cc(x, y, n: int, k: complex, stream=None):
    check(lib().nsh_mul_const_cc(ptr(x), ptr(y), n, float(k.real), float(k.imag), stream_ptr(stream)),
          "nsh_mul_const_cc")


def mul_const_ff(x, y, n: int, k: float, stream=None):
    check(lib().nsh_mul_const_ff(ptr(x), ptr(y), n, float(k), stream_ptr(stream)), "nsh_mul_const_ff")


def mul_const_chain_cc(x, y, n: int, ks, stream=None):
    arr = (C.c_float * (2 * len(ks)))(*[v for k in ks for v in (complex(k).real, complex(k).imag)])
    check(lib().nsh_mul_const_chain_cc(ptr(x), ptr(y), n, arr, len(ks), stream_ptr(stream)),
          "nsh_mul_const_chain_cc")


def add_cc(a, b, y, n: int, stream=None):
    check(lib().nsh_add_cc(ptr(a), ptr(b), ptr(y), n, stream_ptr(stream)), "nsh_add_cc")


def mul_cc(a, b, y, n: int, stream=None):
    check(lib().nsh_mul_cc(ptr(a), ptr(b), ptr(y), n, stream_ptr(stream)), "nsh_mul_cc")


def mul_const_vcc(x, y, k, vlen: int, nitems: int, stream=None):
    """y[i][j] = x[i][j] * k[j] over nitems items of vlen samples (k: device, vlen complex)."""
    check(lib().nsh_mul_const_vcc(ptr(x), ptr(y), ptr(k), vlen, nitems, stream_ptr(stream)), "nsh_mul_const_vcc")


class ClockSampler:
    """nsh_clock_sample on a side stream: start() before the work to observe, mhz() after it
    (waits for the sample). One wave sleeping between two counter reads, ~real_ms long."""

    def __init__(self, real_ms: float = 8.0):
        import torch

        self._ticks = max(1, int(real_ms * 1e5))  # 100 MHz real-time counter
        self._out = torch.zeros(2, dtype=torch.int64, device="cuda")
        self._s = torch.cuda.Stream()

    def start(self):
        check(lib().nsh_clock_sample(ptr(self._out), self._ticks, stream_ptr(self._s)), "nsh_clock_sample")

    def mhz(self) -> float:
        self._s.synchronize()
        cyc, ticks = (int(v) for v in self._out.cpu().tolist())
        return 100.0 * cyc / ticks if ticks > 0 else float("nan")


def synth(y, n: int, first_index: int = 0, seed: int = 0x6E736368, stream=None):
    check(lib().nsh_synth_cf32(ptr(y), n, first_index, seed, stream_ptr(stream)), "nsh_synth_cf32")


def fft1024(x, y, nframes: int, inverse: bool = False, stream=None):
    check(lib().nsh_fft1024_c2c(ptr(x), ptr(y), nframes, 1 if inverse else 0, stream_ptr(stream)),
          "nsh_fft1024_c2c")


def channelizer1024(x, y, w, nframes: int, stream=None):
    check(lib().nsh_channelizer1024(ptr(x), ptr(y), ptr(w), nframes, stream_ptr(stream)),
          "nsh_channelizer1024")


class _Plan:
    """A native plan handle (_h) with the C function that destroys it (_destroy, by name)."""

    _destroy = ""
    _h = None

    @staticmethod
    def _taps_arg(taps):
        """taps as a contiguous float32 array (kept by the caller across the call) and its POINTER(c_float)."""
        import numpy as np

        t = np.ascontiguousarray(np.asarray(taps, dtype=np.float32))
        return t, t.ctypes.data_as(C.POINTER(C.c_float))

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FftPlan(_Plan):
    """FFT of fft_size = 2^k points (16..8192), forward or inverse, unnormalised, with an optional
    real window on the input and an optional half-frame shift, in one launch; see nsh_fft_c2c."""

    _destroy = "nsh_fft_plan_destroy"

    def __init__(self, fft_size: int, inverse: bool = False, window=None, shift: bool = False, device: int = 0):
        self.fft_size = int(fft_size)
        self.inverse = bool(inverse)
        self.shift = bool(shift)
        arr = None
        if window is not None:
            w, arr = self._taps_arg(window)
            if w.size != self.fft_size:
                raise NshError(f"FftPlan: the window has {w.size} entries, fft_size is {self.fft_size}")
        h = C.c_void_p()
        check(lib().nsh_fft_plan_create(device, self.fft_size, 1 if inverse else 0, arr, 1 if shift else 0, C.byref(h)),
              "nsh_fft_plan_create")
        self._h = h
        self.tile = lib().nsh_fft_tile(h)
        self.kernel = lib().nsh_fft_kernel(h).decode()

    def grid_cap(self, max_workgroups: int = 0):
        """At most max_workgroups workgroups per launch (0: the default); the output does not depend on it."""
        check(lib().nsh_fft_plan_grid_cap(self._h, int(max_workgroups)), "nsh_fft_plan_grid_cap")

    def __call__(self, x, y, nframes: int, stream=None):
        check(lib().nsh_fft_c2c(self._h, ptr(x), ptr(y), nframes, stream_ptr(stream)), "nsh_fft_c2c")


def fft_c2c(plan: FftPlan, x, y, nframes: int, stream=None):
    """y = the plan's transform of nframes frames of x (device tensors, complex64 or float32 views)."""
    plan(x, y, nframes, stream)


class FftFilterPlan(_Plan):
    """FIR filter with complex taps by overlap-save in one launch (window -> FFT -> times the taps'
    spectrum -> inverse FFT -> valid part); see nsh_fft_filter_ccc. fft_size 0: chosen by the plan."""

    _destroy = "nsh_fft_filter_plan_destroy"

    def __init__(self, taps, fft_size: int = 0, device: int = 0):
        import numpy as np

        t = np.ascontiguousarray(np.asarray(taps, dtype=np.complex64))
        self.ntaps = int(t.size)
        h = C.c_void_p()
        check(lib().nsh_fft_filter_plan_create(device, t.view(np.float32).ctypes.data_as(C.POINTER(C.c_float)),
                                               self.ntaps, int(fft_size), C.byref(h)), "nsh_fft_filter_plan_create")
        self._h = h
        self.fft_size = lib().nsh_fft_filter_fft_size(h)
        self.valid = lib().nsh_fft_filter_valid(h)
        self.hist_len = lib().nsh_fft_filter_history(h)
        self.tile = lib().nsh_fft_filter_tile(h)
        self.kernel = lib().nsh_fft_filter_kernel(h).decode()

    def grid_cap(self, max_workgroups: int = 0):
        """At most max_workgroups workgroups per launch (0: the default); the output does not depend on it."""
        check(lib().nsh_fft_filter_grid_cap(self._h, int(max_workgroups)), "nsh_fft_filter_grid_cap")

    def __call__(self, x, hist_in, hist_out, y, n: int, stream=None):
        """n outputs from n inputs; hist_in (or None = zeros) / hist_out: ntaps-1 raw samples."""
        check(lib().nsh_fft_filter_ccc(self._h, ptr(x), _opt_ptr(hist_in), _opt_ptr(hist_out), ptr(y), n,
                                       stream_ptr(stream)), "nsh_fft_filter_ccc")


class FftXlatPlan(_Plan):
    """Tune by freq_norm (cycles per input sample), filter with complex taps and decimate by
    decim in {1, 2, ..., 64} by overlap-save in one launch (window -> FFT -> times the band-pass taps'
    spectrum -> fold to fft_size / decim bins -> inverse FFT -> rotate -> valid part); see
    nsh_fft_xlat_ccc. fft_size 0: chosen by the plan."""

    _destroy = "nsh_fft_xlat_plan_destroy"

    def __init__(self, taps, decim: int = 1, freq_norm: float = 0.0, fft_size: int = 0, device: int = 0):
        import numpy as np

        t = np.ascontiguousarray(np.asarray(taps, dtype=np.complex64))
        self.ntaps = int(t.size)
        h = C.c_void_p()
        check(lib().nsh_fft_xlat_plan_create(device, t.view(np.float32).ctypes.data_as(C.POINTER(C.c_float)),
                                             self.ntaps, int(decim), float(freq_norm), int(fft_size), C.byref(h)),
              "nsh_fft_xlat_plan_create")
        self._h = h
        self.fft_size = lib().nsh_fft_xlat_fft_size(h)
        self.decim = lib().nsh_fft_xlat_decim(h)
        self.overlap = lib().nsh_fft_xlat_overlap(h)
        self.valid = lib().nsh_fft_xlat_valid(h)
        self.hist_len = lib().nsh_fft_xlat_history(h)
        self.tile = lib().nsh_fft_xlat_tile(h)
        self.kernel = lib().nsh_fft_xlat_kernel(h).decode()
        inc = C.c_uint64()
        check(lib().nsh_fft_xlat_phase_inc(h, C.byref(inc)), "nsh_fft_xlat_phase_inc")
        self.phase_inc = int(inc.value)

    def grid_cap(self, max_workgroups: int = 0):
        """At most max_workgroups workgroups per launch (0: the default); the output does not depend on it."""
        check(lib().nsh_fft_xlat_grid_cap(self._h, int(max_workgroups)), "nsh_fft_xlat_grid_cap")

    def __call__(self, x, hist_in, hist_out, y, n_out: int, first_index: int = 0, stream=None):
        """n_out outputs from n_out * decim inputs; hist_in (or None = zeros) / hist_out: ntaps-1 raw
        samples; first_index: the absolute stream index of x[0] (mod 2^64)."""
        check(lib().nsh_fft_xlat_ccc(self._h, ptr(x), _opt_ptr(hist_in), _opt_ptr(hist_out), ptr(y), n_out,
                                     first_index & 0xFFFFFFFFFFFFFFFF, stream_ptr(stream)), "nsh_fft_xlat_ccc")


class PsdPlan(_Plan):
    """Spectrum estimate: windowed forward FFT of fft_size points, |X|^2, summed over navg frames and
    scaled (scale None: 1 / navg), optionally shifted and as 10 log10; see nsh_psd_cf. One stream at
    a time: a plan with navg > segment owns scratch memory."""

    _destroy = "nsh_psd_plan_destroy"

    def __init__(self, fft_size: int, navg: int, window=None, shift: bool = False, scale=None, db: bool = False,
                 device: int = 0):
        self.fft_size = int(fft_size)
        self.navg = int(navg)
        self.shift = bool(shift)
        self.db = bool(db)
        self.scale = float(1.0 / max(self.navg, 1) if scale is None else scale)
        arr = None
        if window is not None:
            w, arr = self._taps_arg(window)
            if w.size != self.fft_size:
                raise NshError(f"PsdPlan: the window has {w.size} entries, fft_size is {self.fft_size}")
        h = C.c_void_p()
        check(lib().nsh_psd_plan_create(device, self.fft_size, self.navg, arr, 1 if shift else 0, self.scale,
                                        1 if db else 0, C.byref(h)), "nsh_psd_plan_create")
        self._h = h
        self.segment = lib().nsh_psd_segment(h)
        self.tile = lib().nsh_psd_tile(h)
        self.kernel = lib().nsh_psd_kernel(h).decode()

    def grid_cap(self, max_workgroups: int = 0):
        """At most max_workgroups workgroups per launch (0: the default); the output does not depend on it."""
        check(lib().nsh_psd_grid_cap(self._h, int(max_workgroups)), "nsh_psd_grid_cap")

    def __call__(self, x, y, nvec: int, stream=None):
        """nvec vectors of fft_size floats from nvec * navg * fft_size complex samples."""
        check(lib().nsh_psd_cf(self._h, ptr(x), ptr(y), nvec, stream_ptr(stream)), "nsh_psd_cf")


class FirPlan(_Plan):
    """Device-resident FIR plan (taps uploaded/split once); see nsh_fir_ccf."""

    _destroy = "nsh_fir_plan_destroy"

    def __init__(self, taps, decim: int = 1, algo: int = FIR_AUTO, device: int = 0):
        t, arr = self._taps_arg(taps)
        self.ntaps = int(t.size)
        self.decim = int(decim)
        h = C.c_void_p()
        check(lib().nsh_fir_plan_create(device, arr, self.ntaps, self.decim, algo, C.byref(h)),
              "nsh_fir_plan_create")
        self._h = h
        self.algo = lib().nsh_fir_plan_algo(h)
        self.kernel = lib().nsh_fir_plan_kernel(h).decode()

    def __call__(self, x, hist_in, hist_out, y, n_out: int, stream=None):
        check(lib().nsh_fir_ccf(self._h, ptr(x), ptr(hist_in), ptr(hist_out), ptr(y), n_out,
                                stream_ptr(stream)), "nsh_fir_ccf")


def phase_inc(turns_per_sample: float) -> int:
    """round(frac(t) * 2^64) mod 2^64: the 64-bit phase increment of t turns per sample (nsh_phase_inc)."""
    inc = C.c_uint64(0)
    check(lib().nsh_phase_inc(float(turns_per_sample), C.byref(inc)), "nsh_phase_inc")
    return inc.value


def rotate_cc(x, y, n: int, inc: int, first_index: int = 0, stream=None):
    """y[i] = x[i] * exp(2j pi ((first_index + i) * inc mod 2^64) / 2^64); x may be y (nsh_rotate_cc)."""
    check(lib().nsh_rotate_cc(ptr(x), ptr(y), n, inc & (2**64 - 1), first_index & (2**64 - 1), stream_ptr(stream)),
          "nsh_rotate_cc")


class FirXlatPlan(_Plan):
    """Frequency-translating decimating FIR (rotate -> FIR -> decimate in one kernel); see
    nsh_fir_xlat_ccf. freq_norm = center_freq / samp_rate."""

    _destroy = "nsh_fir_xlat_plan_destroy"

    def __init__(self, taps, decim: int = 1, freq_norm: float = 0.0, device: int = 0):
        t, arr = self._taps_arg(taps)
        self.ntaps = int(t.size)
        self.decim = int(decim)
        h = C.c_void_p()
        check(lib().nsh_fir_xlat_plan_create(device, arr, self.ntaps, self.decim, float(freq_norm), C.byref(h)),
              "nsh_fir_xlat_plan_create")
        self._h = h
        inc = C.c_uint64(0)
        check(lib().nsh_fir_xlat_phase_inc(h, C.byref(inc)), "nsh_fir_xlat_phase_inc")
        self.inc = inc.value
        self.tile = lib().nsh_fir_xlat_tile(h)
        self.kernel = lib().nsh_fir_xlat_kernel(h).decode()

    def __call__(self, x, hist_in, hist_out, y, n_out: int, first_index: int = 0, stream=None):
        """n_out outputs from n_out * decim inputs; hist_in (or None = zeros) / hist_out: ntaps-1 raw samples."""
        check(lib().nsh_fir_xlat_ccf(self._h, ptr(x), _opt_ptr(hist_in), _opt_ptr(hist_out), ptr(y), n_out,
                                     first_index & (2**64 - 1), stream_ptr(stream)), "nsh_fir_xlat_ccf")


class PfbPlan(_Plan):
    """Critically sampled polyphase filterbank channelizer (nchans branch FIRs and an inverse DFT in
    one kernel); see nsh_pfb_channelizer_ccf."""

    _destroy = "nsh_pfb_plan_destroy"

    def __init__(self, taps, nchans: int, device: int = 0):
        t, arr = self._taps_arg(taps)
        self.ntaps = int(t.size)
        self.nchans = int(nchans)
        h = C.c_void_p()
        check(lib().nsh_pfb_plan_create(device, arr, self.ntaps, self.nchans, C.byref(h)), "nsh_pfb_plan_create")
        self._h = h
        self.tile = lib().nsh_pfb_tile(h)
        self.kernel = lib().nsh_pfb_kernel(h).decode()

    def __call__(self, x, hist_in, hist_out, y, n_out: int, stream=None):
        """n_out items of nchans channels from n_out * nchans inputs; hist_in (or None = zeros) /
        hist_out: ntaps-1 raw samples."""
        check(lib().nsh_pfb_channelizer_ccf(self._h, ptr(x), _opt_ptr(hist_in), _opt_ptr(hist_out), ptr(y),
                                            n_out, stream_ptr(stream)), "nsh_pfb_channelizer_ccf")


class PfbSynthPlan(_Plan):
    """Critically sampled polyphase synthesis filterbank, the channelizer's counterpart (an inverse
    DFT across the nchans channels of every item and nchans branch FIRs in one kernel); see
    nsh_pfb_synthesizer_ccf."""

    _destroy = "nsh_pfb_synth_plan_destroy"

    def __init__(self, taps, nchans: int, device: int = 0):
        t, arr = self._taps_arg(taps)
        self.ntaps = int(t.size)
        self.nchans = int(nchans)
        h = C.c_void_p()
        check(lib().nsh_pfb_synth_plan_create(device, arr, self.ntaps, self.nchans, C.byref(h)),
              "nsh_pfb_synth_plan_create")
        self._h = h
        self.tile = lib().nsh_pfb_synth_tile(h)
        self.kernel = lib().nsh_pfb_synth_kernel(h).decode()

    def __call__(self, x, hist_in, hist_out, y, n_in: int, stream=None):
        """n_in * nchans outputs from n_in items of nchans channels; hist_in (or None = zeros) /
        hist_out: the ceil(ntaps / nchans) - 1 raw items before x."""
        check(lib().nsh_pfb_synthesizer_ccf(self._h, ptr(x), _opt_ptr(hist_in), _opt_ptr(hist_out), ptr(y),
                                            n_in, stream_ptr(stream)), "nsh_pfb_synthesizer_ccf")


class ResampPlan(_Plan):
    """Rational resampler by interp / decim (zero-stuff, FIR, decimate in one kernel); see nsh_resamp_ccf."""

    _destroy = "nsh_resamp_plan_destroy"

    def __init__(self, taps, interp: int, decim: int, device: int = 0):
        t, arr = self._taps_arg(taps)
        self.ntaps = int(t.size)
        self.interp = int(interp)
        self.decim = int(decim)
        h = C.c_void_p()
        check(lib().nsh_resamp_plan_create(device, arr, self.ntaps, self.interp, self.decim, C.byref(h)),
              "nsh_resamp_plan_create")
        self._h = h
        self.tile = lib().nsh_resamp_tile(h)
        self.history = lib().nsh_resamp_history(h)
        self.kernel = lib().nsh_resamp_kernel(h).decode()

    def __call__(self, x, hist_in, hist_out, y, n_units: int, stream=None):
        """n_units * interp outputs from n_units * decim inputs; hist_in (or None = zeros) / hist_out:
        `history` = ceil(ntaps / interp) - 1 raw samples."""
        check(lib().nsh_resamp_ccf(self._h, ptr(x), _opt_ptr(hist_in), _opt_ptr(hist_out), ptr(y), n_units,
                                   stream_ptr(stream)), "nsh_resamp_ccf")


def arb_step(rate: float, nfilt: int = 32) -> int:
    """round(nfilt / rate * 2^32): the Q32.32 step, in filter steps per output, of a rate (nsh_arb_step)."""
    step = C.c_uint64(0)
    check(lib().nsh_arb_step(float(rate), int(nfilt), C.byref(step)), "nsh_arb_step")
    return step.value


def arb_span(step: int, nfilt: int, phase: int, n_in: int, want: int):
    """(n_out, n_consumed, phase_next) of a call with n_in inputs from phase that wants `want` outputs
    (nsh_arb_span; host only)."""
    n_out, c, nxt = C.c_int64(0), C.c_int64(0), C.c_uint64(0)
    check(lib().nsh_arb_span(step, int(nfilt), phase, n_in, want, C.byref(n_out), C.byref(c), C.byref(nxt)),
          "nsh_arb_span")
    return n_out.value, c.value, nxt.value


class ArbPlan(_Plan):
    """Arbitrary-rate polyphase resampler (nfilt filters and their derivative filters, exact integer
    phase, one kernel); see nsh_arb_resamp_ccf."""

    _destroy = "nsh_arb_plan_destroy"

    def __init__(self, taps, rate: float, nfilt: int = 32, device: int = 0):
        t, arr = self._taps_arg(taps)
        self.ntaps = int(t.size)
        self.nfilt = int(nfilt)
        h = C.c_void_p()
        check(lib().nsh_arb_plan_create(device, arr, self.ntaps, self.nfilt, float(rate), C.byref(h)),
              "nsh_arb_plan_create")
        self._h = h
        step = C.c_uint64(0)
        check(lib().nsh_arb_plan_step(h, C.byref(step)), "nsh_arb_plan_step")
        self.step = step.value
        self.rate_effective = self.nfilt * 2.0**32 / self.step
        self.tile = lib().nsh_arb_tile(h)
        self.history = lib().nsh_arb_history(h)
        self.kernel = lib().nsh_arb_kernel(h).decode()

    def span(self, phase: int, n_in: int, want: int):
        """(n_out, n_consumed, phase_next): what a call with n_in inputs from phase can make of `want`."""
        return arb_span(self.step, self.nfilt, phase, n_in, want)

    def __call__(self, x, n_in: int, hist_in, hist_out, y, n_out: int, phase: int = 0, stream=None):
        """n_out outputs (at most span(phase, n_in, ...)) from n_in inputs; hist_in (or None = zeros) /
        hist_out: `history` = ceil(ntaps / nfilt) - 1 raw samples. n_out = 0 only advances."""
        check(lib().nsh_arb_resamp_ccf(self._h, ptr(x), n_in, _opt_ptr(hist_in), _opt_ptr(hist_out),
                                       _opt_ptr(y), n_out, phase, stream_ptr(stream)), "nsh_arb_resamp_ccf")


class FirCascadePlan(_Plan):
    """A chain of fir_filter_ccf(taps_s, decim_s) stages as one pass; see nsh_fir_cascade_ccf."""

    _destroy = "nsh_fir_cascade_plan_destroy"

    def __init__(self, stages, device: int = 0):
        taps = [self._taps_arg(t) for t, _ in stages]
        n = len(taps)
        tp = (C.POINTER(C.c_float) * n)(*[arr for _, arr in taps])
        nt = (C.c_int * n)(*[int(t.size) for t, _ in taps])
        dc = (C.c_int * n)(*[int(d) for _, d in stages])
        h = C.c_void_p()
        check(lib().nsh_fir_cascade_plan_create(device, tp, nt, dc, n, C.byref(h)), "nsh_fir_cascade_plan_create")
        self._h = h
        self.decim = lib().nsh_fir_cascade_decim(h)
        self.hist_len = lib().nsh_fir_cascade_hist_len(h)
        self.kernel = lib().nsh_fir_cascade_kernel(h).decode()

    def __call__(self, x, hist_in, hist_out, y, n_out: int, stream=None):
        """n_out outputs from n_out * decim inputs; hist_in/hist_out: hist_len samples (or 0/None)."""
        check(lib().nsh_fir_cascade_ccf(self._h, _opt_ptr(x), _opt_ptr(hist_in), _opt_ptr(hist_out), ptr(y),
                                        n_out, stream_ptr(stream)), "nsh_fir_cascade_ccf")
