"""GPU: nsh_resamp_ccf (k_resamp<R,P>) through the C-ABI.

Reference for every numeric check: resamp_ref below, numpy complex128 straight from the definition
(zero-stuff by I, convolve, keep every D-th), judged with oracle.tol_ok at 1e-5. A numpy fp32
emulation of the kernel's q-ascending accumulation stays within 1.0e-6 of it over CASES (worst at
Q = 1024 taps per output), so the contract has a tenfold margin for a correct fp32 kernel."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from newsched_amd import nsh
from tests.fir_accuracy import resamp_ref_conv as resamp_ref
from tests.gpu_util import assert_tol, dev, host, windowed_sinc

pytestmark = pytest.mark.gpu


def taps_for(L, I, D):
    """Windowed sinc for resampling by I / D, gain I."""
    return windowed_sinc(L, max(I, D), I)


@pytest.fixture(scope="module")
def stream():
    return orc.synth(1 << 17, 2024)


def run_resamp(torch, plan, x, hist, n_units, in_off=0, out_off=0, stream=None):
    """One call; returns (y, hist_out). hist None = NULL hist_in. Guard words around the output."""
    I, D, H = plan.interp, plan.decim, plan.history
    n_in, n_out = n_units * D, n_units * I
    buf = np.zeros(n_in + 2, np.complex64)
    buf[in_off:in_off + n_in] = x[:n_in]
    dx = dev(torch, buf)
    dh = dev(torch, hist) if hist is not None and H > 0 else None
    dho = torch.full((max(H, 1),), 5 + 5j, dtype=torch.complex64, device="cuda")
    dy = torch.full((n_out + 6,), 9 - 9j, dtype=torch.complex64, device="cuda")
    o = 2 + out_off                                   # guard words before and after the output
    plan(dx.data_ptr() + 8 * in_off, dh, dho, dy.data_ptr() + 8 * o, n_units, stream=stream)
    y = host(dy)
    assert np.all(y[:o] == 9 - 9j) and np.all(y[o + n_out:] == 9 - 9j)  # nothing outside n_out
    return y[o:o + n_out], host(dho)[:H]


def instantiation(I, D):
    return "8,1" if D <= I else "8,0" if D <= 2 * I else "4,0" if D <= 4 * I else "2,0" if D <= 8 * I else "1,0"


# (I, D, L, units)
CASES = [(1, 1, 1, 1000), (2, 1, 15, 1000), (3, 2, 64, 777), (4, 1, 127, 1000), (3, 5, 95, 1000), (5, 3, 1, 333),
         (7, 64, 1024, 200), (64, 1, 1024, 1000), (64, 63, 1000, 100), (48, 25, 601, 300), (1, 4, 1024, 1000),
         (2, 3, 1024, 1000), (10, 1, 3, 1000), (63, 64, 63, 200)]


@pytest.mark.parametrize("case", CASES, ids=[f"I{i}-D{d}-L{l}-n{n}" for i, d, l, n in CASES])
@pytest.mark.parametrize("with_hist", [True, False], ids=["hist", "nullhist"])
def test_resamp_cases(torch_cuda, stream, case, with_hist):
    torch = torch_cuda
    I, D, L, n_units = case
    taps = taps_for(L, I, D)
    plan = nsh.ResampPlan(taps, I, D)
    H = -(-L // I) - 1
    assert plan.kernel == f"k_resamp<{instantiation(I, D)}>" and plan.history == H
    assert (plan.ntaps, plan.interp, plan.decim) == (L, I, D) and plan.tile >= 1
    x = stream[2000:2000 + n_units * D]
    hist = stream[2000 - H:2000].copy() if with_hist else None
    y, ho = run_resamp(torch, plan, x, hist, n_units)
    assert_tol(y, resamp_ref(x, hist, taps, I, D, n_units), f"{plan.kernel} I={I} D={D} L={L}")
    raw = np.concatenate([hist if hist is not None else np.zeros(H, np.complex64), x])
    np.testing.assert_array_equal(ho, raw[raw.size - H:])
    plan.close()


# one plan per instantiation, and the widest interpolator
@pytest.mark.parametrize("I,D,L", [(3, 2, 95), (2, 3, 95), (1, 4, 63), (1, 8, 63), (1, 64, 200), (64, 1, 1024)])
def test_resamp_tile_edges(torch_cuda, I, D, L):
    torch = torch_cuda
    taps = taps_for(L, I, D)
    plan = nsh.ResampPlan(taps, I, D)
    U, H = plan.tile, plan.history
    x = orc.synth((3 * U + 1) * D + H, 55)
    hist, x = x[:H].copy(), x[H:]
    ref = resamp_ref(x, hist, taps, I, D, 3 * U + 1)
    for n_units in (U - 1, U, U + 1, 3 * U + 1):
        y, _ = run_resamp(torch, plan, x, hist, n_units)
        assert_tol(y, ref[:n_units * I], f"{plan.kernel} tile={U} n_units={n_units}")
    plan.close()


@pytest.mark.parametrize("I,D", [(3, 2), (4, 5)])
@pytest.mark.parametrize("in_off,out_off", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_resamp_pointers_offset_by_8_bytes(torch_cuda, stream, I, D, in_off, out_off):
    torch = torch_cuda
    L, n_units = 95, 1501
    taps = taps_for(L, I, D)
    plan = nsh.ResampPlan(taps, I, D)
    H = plan.history
    x = stream[:n_units * D]
    hist = stream[-H:].copy()
    y, ho = run_resamp(torch, plan, x, hist, n_units, in_off=in_off, out_off=out_off)
    assert_tol(y, resamp_ref(x, hist, taps, I, D, n_units), f"in at {8 * in_off} mod 16, out at {8 * out_off} mod 16")
    np.testing.assert_array_equal(ho, x[-H:])
    plan.close()


@pytest.mark.parametrize("I,D,L", [(3, 2, 95), (4, 5, 159), (1, 4, 127), (1, 8, 63), (1, 64, 1024)])
def test_resamp_chunked_stream_is_bit_identical(torch_cuda, stream, I, D, L):
    torch = torch_cuda
    taps = taps_for(L, I, D)
    plan = nsh.ResampPlan(taps, I, D)
    U = plan.tile
    total = 2 * U + 50
    x = stream[:total * D]
    whole, hw = run_resamp(torch, plan, x, None, total)
    out, hist, pos = [], None, 0
    for n_units in (1, U - 1, 2, total - U - 2):
        y, hist = run_resamp(torch, plan, x[pos * D:], hist, n_units, out_off=pos & 1)
        out.append(y)
        pos += n_units
    assert pos == total
    y = np.concatenate(out)
    np.testing.assert_array_equal(y.view(np.uint32), whole.view(np.uint32))
    np.testing.assert_array_equal(hist, hw)
    assert_tol(y, resamp_ref(x, None, taps, I, D, total), "chunked vs reference")
    plan.close()


def test_resamp_phases_of_an_interpolator(torch_cuda, stream):
    """D = 1: output phase r is the input filtered by the taps h[r::I]."""
    torch = torch_cuda
    I, L, n_units = 5, 98, 2000
    taps = taps_for(L, I, 1)
    plan = nsh.ResampPlan(taps, I, 1)
    x = stream[:n_units]
    y, _ = run_resamp(torch, plan, x, None, n_units)
    for r in range(I):
        assert_tol(y[r::I], resamp_ref(x, None, taps[r::I], 1, 1, n_units), f"phase {r} of {I}")
    plan.close()


@pytest.mark.parametrize("D,L", [(1, 63), (4, 127), (64, 1024)])
def test_resamp_without_interpolation_equals_the_translating_fir(torch_cuda, stream, D, L):
    torch = torch_cuda
    n_units = 1500
    taps = taps_for(L, 1, D)
    plan = nsh.ResampPlan(taps, 1, D)
    x = stream[5000:5000 + n_units * D]
    hist = stream[5000 - (L - 1):5000].copy()
    y, _ = run_resamp(torch, plan, x, hist, n_units)
    xl = nsh.FirXlatPlan(taps, D, 0.0)
    dho = torch.empty(L - 1, dtype=torch.complex64, device="cuda")
    dy = torch.empty(n_units, dtype=torch.complex64, device="cuda")
    xl(dev(torch, x), dev(torch, hist), dho, dy, n_units, 0)
    assert_tol(y, host(dy), f"{plan.kernel} vs {xl.kernel}")
    assert_tol(y, resamp_ref(x, hist, taps, 1, D, n_units), "vs reference")
    xl.close()
    plan.close()


# (4, 3, 30): L is no multiple of I, so phases 2 and 3 have one tap fewer than Q = 8 and their last
# row is the padding; (64, 63, 1000): 24 padded taps; (1, 4, 63): a plain decimator
@pytest.mark.parametrize("I,D,L", [(4, 3, 30), (64, 63, 1000), (1, 4, 63), (3, 1, 7)])
@pytest.mark.parametrize("spike", [complex(np.nan, np.nan), complex(np.inf, 0)], ids=["nan", "inf"])
def test_resamp_non_finite_reaches_exactly_its_outputs(torch_cuda, stream, I, D, L, spike):
    torch = torch_cuda
    n_units = 400
    taps = taps_for(L, I, D)
    assert np.all(taps != 0)
    plan = nsh.ResampPlan(taps, I, D)
    x = stream[:n_units * D].copy()
    clean, _ = run_resamp(torch, plan, x, None, n_units)
    j = 150 * D + 1 if D > 1 else 150
    x[j] = spike
    y, _ = run_resamp(torch, plan, x, None, n_units)
    n = np.arange(n_units * I)
    k = n * D - j * I                                  # the tap that meets sample j in output n
    hit = (k >= 0) & (k < L)
    assert 0 < hit.sum() <= -(-L // D) and hit.sum() >= L // D
    bad = ~(np.isfinite(y.real) & np.isfinite(y.imag))
    np.testing.assert_array_equal(bad, hit)
    np.testing.assert_array_equal(y[~hit].view(np.uint32), clean[~hit].view(np.uint32))
    plan.close()


def test_resamp_requires_hist_out(torch_cuda):
    torch = torch_cuda
    plan = nsh.ResampPlan(np.ones(4, np.float32), 2, 3)
    d = torch.zeros(64, dtype=torch.complex64, device="cuda")
    dy = torch.zeros(64, dtype=torch.complex64, device="cuda")
    with pytest.raises(nsh.NshError, match="hist_out is required"):
        plan(d, None, None, dy, 8)
    one = nsh.ResampPlan(np.ones(2, np.float32), 2, 3)   # Q = 1: no history at all
    assert one.history == 0
    one(d, None, None, dy, 8)
    torch.cuda.synchronize()
    plan.close()
    one.close()


def test_resamp_two_streams_give_the_same_bits(torch_cuda, stream):
    torch = torch_cuda
    I, D, L, n_units = 4, 5, 159, 3000
    plan = nsh.ResampPlan(taps_for(L, I, D), I, D)
    x = stream[:n_units * D]
    ya, _ = run_resamp(torch, plan, x, None, n_units)
    s = torch.cuda.Stream()
    yb, _ = run_resamp(torch, plan, x, None, n_units, stream=s)
    np.testing.assert_array_equal(ya.view(np.uint32), yb.view(np.uint32))
    plan.close()


def test_resamp_armed_pair_taken_by_exactly_one_launch(torch_cuda, stream):
    torch = torch_cuda
    L = nsh.lib()

    def timed(call):
        ev = [C.c_void_p(), C.c_void_p()]
        for e in ev:
            nsh.check(L.nsh_event_create(C.byref(e)))
        before, after = C.c_uint64(0), C.c_uint64(0)
        nsh.check(L.nsh_timed_launches(C.byref(before)))
        nsh.check(L.nsh_time_next_launch(ev[0], ev[1]))
        call()
        nsh.check(L.nsh_timed_launches(C.byref(after)))
        torch.cuda.synchronize()
        ms = C.c_float(-1)
        rc = L.nsh_event_elapsed_ms(ev[0], ev[1], C.byref(ms))
        for e in ev:
            L.nsh_event_destroy(e)
        return after.value - before.value, rc, ms.value

    I, D, n_units = 3, 2, 4099
    dx = dev(torch, stream[:n_units * D + 2])
    dy = torch.full((n_units * I + 2,), 9 - 9j, dtype=torch.complex64, device="cuda")
    plan = nsh.ResampPlan(taps_for(95, I, D), I, D)
    dh = torch.zeros(max(plan.history, 1), dtype=torch.complex64, device="cuda")
    count, rc, ms = timed(lambda: plan(dx.data_ptr() + 8, None, dh, dy, n_units))
    assert count == 1 and rc == 0 and ms >= 0
    count, rc, ms = timed(lambda: plan(dx, None, dh, dy.data_ptr() + 8, n_units))   # the 8-byte store path
    assert count == 1 and rc == 0 and ms >= 0
    dy.fill_(9 - 9j)
    count, rc, _ = timed(lambda: plan(dx, None, dh, dy, 0))   # zero units: nothing launched, the pair dropped unrecorded
    assert count == 0 and rc != 0
    assert np.all(host(dy) == 9 - 9j)
    plan.close()
