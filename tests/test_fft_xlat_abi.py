"""CPU: the C-ABI of freq_xlating_fft_filter_ccc (nsh_fft_xlat_plan_create .. nsh_fft_xlat_ccc) where
it needs no GPU: every refusal happens before any HIP call, in the header's order, and leaves its
message in nsh_last_error; n_out <= 0 is a no-op whatever the pointers; the accessors answer 0 or ""
for a NULL plan (the binding's signatures against the header: tests/test_abi.py); a plan's N, O, V and phase increment
against the Python model (a plan made where there is no device keeps its tables on the host); and the
float64 reference of tests/test_gpu_fft_xlat.py against a term-by-term double sum."""
import ctypes as C

import numpy as np
import pytest

from newsched_amd import nsh
from tests import fft_xlat_ref as ref
from tests.gpu_util import ONE, TWO, refused

THREE, FOUR = C.c_void_p(48), C.c_void_p(64)
BAD_SIZE = b"nsh_fft_xlat_plan_create: fft_size must be 0, 1024, 2048, 4096 or 8192"
BAD_DECIM = b"nsh_fft_xlat_plan_create: decimation must be a power of two in [1, 64]"


def create(taps, decim=1, freq=0.0, fft_size=0, ntaps=None, out=True, null_taps=False):
    h = C.c_void_p()
    t = np.ascontiguousarray(taps, np.complex64)
    arr = None if null_taps else t.view(np.float32).ctypes.data_as(C.POINTER(C.c_float))
    rc = nsh.lib().nsh_fft_xlat_plan_create(0, arr, t.size if ntaps is None else ntaps, decim, freq, fft_size,
                                            C.byref(h) if out else None)
    return rc, h


def test_abi_version_is_unchanged():
    assert nsh.lib().nsh_abi_version() == 1


def test_create_refuses_null_pointers_first():
    # ... before the tap count, the taps, the decimation, the frequency and the size are looked at
    for kw in (dict(null_taps=True), dict(out=False)):
        rc, _ = create(np.full(4, np.nan), decim=3, freq=np.nan, fft_size=7, ntaps=-3, **kw)
        refused(rc, b"nsh_fft_xlat_plan_create: null pointer")


@pytest.mark.parametrize("ntaps", [0, -1, 4097, 1 << 20])
def test_create_refuses_tap_counts(ntaps):
    rc, h = create(np.full(4, np.nan), decim=3, freq=np.nan, fft_size=7, ntaps=ntaps)
    refused(rc, b"nsh_fft_xlat_plan_create: ntaps must be in [1, 4096]")
    assert not h.value


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("L,at,part", [(1, 0, 0), (127, 126, 1), (4096, 2048, 0)])
def test_create_refuses_nonfinite_taps(bad, L, at, part):
    t = np.ones(L, np.complex64)
    t[at] = complex(bad, 1.0) if part == 0 else complex(1.0, bad)
    rc, h = create(t, decim=3, freq=np.nan, fft_size=7)  # ... before the bad decimation
    refused(rc, b"nsh_fft_xlat_plan_create: tap is not finite")
    assert not h.value


@pytest.mark.parametrize("decim", [0, -2, 3, 5, 6, 12, 24, 63, 65, 128, 1 << 20])
def test_create_refuses_decimations(decim):
    rc, h = create(np.ones(4000), decim=decim, freq=np.nan, fft_size=7)  # ... before the bad frequency
    refused(rc, BAD_DECIM)
    assert not h.value


@pytest.mark.parametrize("freq", [np.nan, np.inf, -np.inf])
def test_create_refuses_nonfinite_frequencies(freq):
    rc, h = create(np.ones(4000), decim=4, freq=freq, fft_size=7)  # ... before the bad size
    refused(rc, b"nsh_fft_xlat_plan_create: the frequency must be finite")
    assert not h.value


@pytest.mark.parametrize("size", [-1024, 1, 16, 512, 1000, 1025, 3072, 16384, 1 << 20])
def test_create_refuses_sizes(size):
    rc, h = create(np.ones(4000), decim=4, freq=0.1, fft_size=size)  # ... before ntaps > fft_size / 2
    refused(rc, BAD_SIZE)
    assert not h.value


@pytest.mark.parametrize("size,L", [(1024, 513), (2048, 1025), (4096, 2049), (4096, 4096), (1024, 4096)])
def test_create_refuses_taps_longer_than_half_a_frame(size, L):
    rc, h = create(np.ones(L), decim=2, freq=0.1, fft_size=size)
    refused(rc, b"nsh_fft_xlat_plan_create: ntaps must be at most fft_size / 2")
    assert not h.value


def test_run_refusals_in_order():
    run = nsh.lib().nsh_fft_xlat_ccc
    # NULL in / out, whatever else is wrong
    refused(run(None, None, ONE, ONE, None, 1, 0, None), b"nsh_fft_xlat_ccc: null input or output")
    refused(run(None, ONE, ONE, ONE, None, 1, 0, None), b"nsh_fft_xlat_ccc: null input or output")
    # then in == out, before the histories
    refused(run(None, ONE, THREE, THREE, ONE, 1, 0, None), b"nsh_fft_xlat_ccc: in-place not supported")
    # then aliased histories, before the plan
    refused(run(None, ONE, THREE, THREE, TWO, 1, 0, None), b"nsh_fft_xlat_ccc: hist_out must not alias hist_in")
    # then the NULL plan (two NULL histories alias nothing)
    refused(run(None, ONE, None, None, TWO, 1, 0, None), b"nsh_fft_xlat_ccc: null plan")
    refused(run(None, ONE, THREE, FOUR, TWO, 1, 0, None), b"nsh_fft_xlat_ccc: null plan")


def test_run_refusals_that_need_a_plan():
    """The missing hist_out, then n_out * D too large: both before any HIP call."""
    run = nsh.lib().nsh_fft_xlat_ccc
    rc, h = create(np.ones(2), decim=64)
    assert rc == 0
    refused(run(h, ONE, None, None, TWO, (1 << 62), 0, None), b"nsh_fft_xlat_ccc: hist_out is required")
    refused(run(h, ONE, None, THREE, TWO, (1 << 62), 0, None), b"nsh_fft_xlat_ccc: too many samples for one call")
    refused(run(h, ONE, None, THREE, TWO, (1 << 63) // 16 // 64, 0, None), b"nsh_fft_xlat_ccc: too many samples")
    assert nsh.lib().nsh_fft_xlat_plan_destroy(h) == 0


def test_grid_cap_refusals():
    L = nsh.lib()
    refused(L.nsh_fft_xlat_grid_cap(None, -1), b"nsh_fft_xlat_grid_cap: negative cap")
    refused(L.nsh_fft_xlat_grid_cap(None, 2), b"nsh_fft_xlat_grid_cap: null plan")
    refused(L.nsh_fft_xlat_grid_cap(None, 0), b"nsh_fft_xlat_grid_cap: null plan")


@pytest.mark.parametrize("n", [0, -1, -(1 << 40)])
def test_no_outputs_is_a_no_op_with_any_pointers(n):
    L = nsh.lib()
    for plan, a, hi, ho, b in ((None, None, None, None, None), (None, ONE, TWO, TWO, ONE), (ONE, None, None, None, None),
                               (None, ONE, None, None, TWO)):
        assert L.nsh_fft_xlat_ccc(plan, a, hi, ho, b, n, 5, None) == 0


def test_null_plan_accessors():
    L = nsh.lib()
    assert L.nsh_fft_xlat_fft_size(None) == 0
    assert L.nsh_fft_xlat_decim(None) == 0
    assert L.nsh_fft_xlat_overlap(None) == 0
    assert L.nsh_fft_xlat_valid(None) == 0
    assert L.nsh_fft_xlat_history(None) == 0
    assert L.nsh_fft_xlat_tile(None) == 0
    assert L.nsh_fft_xlat_kernel(None) == b""
    assert L.nsh_fft_xlat_plan_destroy(None) == 0
    inc = C.c_uint64()
    refused(L.nsh_fft_xlat_phase_inc(None, C.byref(inc)), b"nsh_fft_xlat_phase_inc: null pointer")
    refused(L.nsh_fft_xlat_phase_inc(ONE, None), b"nsh_fft_xlat_phase_inc: null pointer")


def test_plan_class_raises_what_the_plan_refuses():
    with pytest.raises(nsh.NshError, match="ntaps must be at most fft_size / 2"):
        nsh.FftXlatPlan(np.ones(600, np.complex64), 2, 0.1, fft_size=1024)
    with pytest.raises(nsh.NshError, match="fft_size must be 0, 1024"):
        nsh.FftXlatPlan(np.ones(3, np.complex64), 2, 0.1, fft_size=512)
    with pytest.raises(nsh.NshError, match="tap is not finite"):
        nsh.FftXlatPlan(np.array([1, np.nan], np.complex64), 2, 0.1)
    with pytest.raises(nsh.NshError, match="decimation must be a power of two"):
        nsh.FftXlatPlan(np.ones(3, np.complex64), 3, 0.1)
    with pytest.raises(nsh.NshError, match="the frequency must be finite"):
        nsh.FftXlatPlan(np.ones(3, np.complex64), 2, float("inf"))


# (L, D, freq_norm, fft_size): L - 1 a multiple of D, one past a multiple, L = 1, L = N / 2, every
# size through the rule and through the override, both signs and more than a turn of frequency
GEOMETRY = [
    (1, 1, 0.0, 0), (1, 64, 0.25, 0), (1, 8, -0.1, 8192),
    (129, 8, 0.1, 0), (129, 64, 0.1, 0), (130, 8, -0.37, 0), (130, 64, 1.25, 2048), (127, 4, 0.123, 0),
    (256, 16, 0.5, 0), (257, 16, -0.5, 0), (257, 32, 1e-9, 0),
    (512, 2, 0.3, 1024), (512, 64, 0.3, 1024), (1024, 32, -2.75, 2048), (513, 2, 0.7, 0),
    (2048, 64, 0.01, 4096), (2048, 1, 0.01, 0), (2049, 4, 0.49, 0), (4096, 64, -0.49, 8192), (4096, 16, 0.2, 0),
]


@pytest.mark.parametrize("L,D,freq,size", GEOMETRY)
def test_plan_geometry_against_the_model(L, D, freq, size):
    p = nsh.FftXlatPlan(np.ones(L, np.complex64), D, freq, fft_size=size)
    N, O, V = ref.geometry(L, D, size)
    assert O % D == 0 and V % D == 0 and 0 <= O - (L - 1) < D and O <= N // 2 and N // D >= 16
    assert (p.fft_size, p.decim, p.overlap, p.valid, p.hist_len) == (N, D, O, V, L - 1)
    assert p.kernel == f"k_fft_xlat<{N}, {D}>"
    assert p.tile == max(1, 4096 // N)
    assert p.phase_inc == ref.phase_inc(-freq)
    inc = C.c_uint64()
    assert nsh.lib().nsh_phase_inc(-freq, C.byref(inc)) == 0 and inc.value == p.phase_inc
    p.grid_cap(3)
    p.grid_cap(0)
    with pytest.raises(nsh.NshError, match="negative cap"):
        p.grid_cap(-1)
    p.close()


@pytest.mark.parametrize("L,D,first,with_hist", [(1, 1, 0, False), (5, 2, 3, True), (7, 4, (1 << 64) - 9, True),
                                                 (40, 8, (1 << 40) + 3, False)])
def test_reference_against_the_term_by_term_sum(L, D, first, with_hist):
    r = np.random.default_rng(L)
    cplx = lambda n: (r.uniform(-1, 1, n) + 1j * r.uniform(-1, 1, n)).astype(np.complex64)
    x, h = cplx(24 * D), cplx(L)
    hist = cplx(L - 1) if with_hist else None
    inc = ref.phase_inc(-0.1371)
    a = ref.ref64(x, h, D, inc, first, hist)
    b = ref.brute64(x, h, D, inc, first, hist)
    assert a.shape == b.shape == (24,)
    assert np.max(np.abs(a - b)) <= 1e-12 * np.abs(h).sum()


def test_complex64_model_stays_inside_the_bound():
    """The numpy / scipy complex64 model of the chain on a small case of every decimation: the bound
    has room for a good fp32 transform (DESIGN.md section 4.10 has the ratios on the GPU tests' inputs)."""
    r = np.random.default_rng(3)
    for D in ref.DECIMS:
        L, N = 127, 1024
        _, O, V = ref.geometry(L, D, N)
        x = (r.uniform(-1, 1, 3 * V + D) + 1j * r.uniform(-1, 1, 3 * V + D)).astype(np.complex64)
        h = (r.uniform(-1, 1, L) + 1j * r.uniform(-1, 1, L)).astype(np.complex64)
        inc = ref.phase_inc(-0.2)
        yr = ref.ref64(x, h, D, inc, 77)
        w = ref.worst(ref.model_c64(x, h, D, N, inc, 77), yr, ref.bound(x, h, D, N, yr))
        assert w <= 0.5, (D, w)
