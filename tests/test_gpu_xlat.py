"""GPU: nsh_rotate_cc (k_rotate) and nsh_fir_xlat_ccf (k_fir_xlat<R,S>) through the C-ABI.

Reference for every numeric check, computed here in numpy complex128: the phase of stream sample n
is (n * inc) mod 2^64 in uint64 wrap-around arithmetic, its top 53 bits / 2^53 turns through
np.exp(2j pi turns); np.convolve with the taps in float64; every D-th output. Judged with
oracle.tol_ok (1e-5), the project's tolerance."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from newsched_amd import nsh
from tests.fir_accuracy import phasors, xlat_ref
from tests.gpu_util import assert_tol, dev, host, windowed_sinc

pytestmark = pytest.mark.gpu

FREQS = [0.1, -0.37, 0.25, 1e-9, 0.4999999]
BIG = 2**40 + 7


def taps_for(L, D):
    return windowed_sinc(L, D)


@pytest.fixture(scope="module")
def stream():
    return orc.synth(1 << 17, 2024)


# ---- rotator ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 4099])
@pytest.mark.parametrize("off_in,off_out", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_rotate_sizes_and_alignment(torch_cuda, stream, n, off_in, off_out):
    torch = torch_cuda
    inc = nsh.phase_inc(0.1)
    x = stream[:n + 4]
    dx = dev(torch, x)
    dy = torch.full((n + 4,), 7 - 3j, dtype=torch.complex64, device="cuda")
    nsh.rotate_cc(dx.data_ptr() + 8 * off_in, dy.data_ptr() + 8 * off_out, n, inc, 12345)
    y = host(dy)
    ref = x[off_in:off_in + n] * phasors(12345, n, inc)
    assert_tol(y[off_out:off_out + n], ref, f"rotate n={n}")
    # samples beyond n (and before the offset) are untouched
    assert np.all(y[:off_out] == 7 - 3j) and np.all(y[off_out + n:] == 7 - 3j)


@pytest.mark.parametrize("f", FREQS)
@pytest.mark.parametrize("first", [0, 12345, BIG])
def test_rotate_frequencies_and_stream_position(torch_cuda, stream, f, first):
    torch = torch_cuda
    n = 4099
    inc = nsh.phase_inc(f)
    dx = dev(torch, stream[:n])
    dy = torch.empty_like(dx)
    nsh.rotate_cc(dx, dy, n, inc, first)
    assert_tol(host(dy), stream[:n] * phasors(first, n, inc), f"rotate f={f} first={first}")


def test_rotate_zero_frequency_is_identity(torch_cuda, stream):
    torch = torch_cuda
    n = 4099
    assert nsh.phase_inc(0.0) == 0
    dx = dev(torch, stream[:n])
    dy = torch.empty_like(dx)
    nsh.rotate_cc(dx, dy, n, 0, BIG)
    np.testing.assert_array_equal(host(dy), stream[:n])


@pytest.mark.parametrize("off", [0, 1])
def test_rotate_in_place_equals_out_of_place(torch_cuda, stream, off):
    torch = torch_cuda
    n = 4099
    inc = nsh.phase_inc(-0.37)
    dx = dev(torch, stream[:n + 2])
    dy = torch.empty_like(dx)
    nsh.rotate_cc(dx.data_ptr() + 8 * off, dy.data_ptr() + 8 * off, n, inc, BIG)
    nsh.rotate_cc(dx.data_ptr() + 8 * off, dx.data_ptr() + 8 * off, n, inc, BIG)
    np.testing.assert_array_equal(host(dx)[off:off + n], host(dy)[off:off + n])


# ---- fused rotate -> FIR -> decimate -------------------------------------------------------------
CASES = [(1, 1, 1), (1, 127, 2049), (2, 127, 5), (3, 8, 257), (5, 33, 1000), (8, 127, 2049), (10, 200, 700),
         (16, 9, 1), (16, 127, 4099), (64, 2, 300), (64, 1024, 257), (7, 1024, 3)]


def run_xlat(torch, plan, x, hist, n_out, first, in_off=0):
    """One call; returns (y, hist_out). hist None = NULL hist_in."""
    L, D = plan.ntaps, plan.decim
    buf = np.zeros(n_out * D + 2, np.complex64)
    buf[in_off:in_off + n_out * D] = x[:n_out * D]
    dx = dev(torch, buf)
    dh = dev(torch, hist) if hist is not None and L > 1 else None
    dho = torch.full((max(L - 1, 1),), 5 + 5j, dtype=torch.complex64, device="cuda")
    dy = torch.full((n_out + 2,), 9 - 9j, dtype=torch.complex64, device="cuda")
    plan(dx.data_ptr() + 8 * in_off, dh, dho, dy, n_out, first)
    y = host(dy)
    assert np.all(y[n_out:] == 9 - 9j)  # nothing past n_out
    return y[:n_out], host(dho)[:L - 1]


@pytest.mark.parametrize("i,case", list(enumerate(CASES)), ids=[f"D{d}-L{l}-n{n}" for d, l, n in CASES])
@pytest.mark.parametrize("with_hist", [True, False], ids=["hist", "nullhist"])
def test_xlat_cases(torch_cuda, stream, i, case, with_hist):
    torch = torch_cuda
    D, L, n_out = case
    f = FREQS[i % len(FREQS)]
    first = BIG if i % 2 else 0
    taps = taps_for(L, D)
    plan = nsh.FirXlatPlan(taps, D, f)
    assert plan.inc == nsh.phase_inc(-f) and plan.kernel.startswith("k_fir_xlat<") and plan.tile * D <= 8192
    x = stream[2000:2000 + n_out * D]
    hist = stream[2000 - (L - 1):2000].copy() if with_hist else None
    y, ho = run_xlat(torch, plan, x, hist, n_out, first)
    assert_tol(y, xlat_ref(x, hist, taps, D, plan.inc, first, n_out), f"{plan.kernel} D={D} L={L}")
    raw = np.concatenate([hist if hist is not None else np.zeros(L - 1, np.complex64), x])
    np.testing.assert_array_equal(ho, raw[raw.size - (L - 1):])
    plan.close()


@pytest.mark.parametrize("D,L", [(1, 127), (4, 127), (8, 65), (16, 127), (32, 100), (64, 200)])
def test_xlat_tile_edges(torch_cuda, D, L):
    torch = torch_cuda
    taps = taps_for(L, D)
    plan = nsh.FirXlatPlan(taps, D, -0.37)
    T = plan.tile
    x = orc.synth((3 * T + 1) * D + L - 1, 55)
    hist, x = x[:L - 1].copy(), x[L - 1:]
    ref = xlat_ref(x, hist, taps, D, plan.inc, BIG, 3 * T + 1)
    for n_out in (T - 1, T, T + 1, 3 * T + 1):
        y, _ = run_xlat(torch, plan, x, hist, n_out, BIG)
        assert_tol(y, ref[:n_out], f"{plan.kernel} T={T} n_out={n_out}")
    plan.close()


def test_xlat_chunked_stream_equals_one_call(torch_cuda, stream):
    torch = torch_cuda
    D, L = 5, 33
    taps = taps_for(L, D)
    plan = nsh.FirXlatPlan(taps, D, 0.1)
    x = stream[:20000]
    whole, _ = run_xlat(torch, plan, x, None, 4000, BIG)
    out, hist, pos = [], None, 0
    for n_in in (5, 1235, 10, 7000, 20000 - 8250):
        y, hist = run_xlat(torch, plan, x[pos:pos + n_in], hist, n_in // D, BIG + pos)
        out.append(y)
        pos += n_in
    assert pos == 20000
    y = np.concatenate(out)
    assert_tol(y, whole, "chunked vs one call")
    assert_tol(y, xlat_ref(x, None, taps, D, plan.inc, BIG, 4000), "chunked vs reference")
    plan.close()


def test_xlat_input_offset_by_8_bytes(torch_cuda, stream):
    torch = torch_cuda
    D, L, n_out = 8, 127, 2049
    taps = taps_for(L, D)
    plan = nsh.FirXlatPlan(taps, D, 0.25)
    x = stream[:n_out * D]
    hist = stream[-(L - 1):].copy()
    y, ho = run_xlat(torch, plan, x, hist, n_out, 12345, in_off=1)
    assert_tol(y, xlat_ref(x, hist, taps, D, plan.inc, 12345, n_out), "input at 8 mod 16")
    np.testing.assert_array_equal(ho, x[-(L - 1):])
    plan.close()


def test_xlat_nan_reaches_exactly_its_windows(torch_cuda, stream):
    torch = torch_cuda
    D, L, n_out = 8, 127, 600
    taps = taps_for(L, D)
    plan = nsh.FirXlatPlan(taps, D, 0.1)
    x = stream[:n_out * D].copy()
    pos = 2000
    x[pos] = np.nan
    y, _ = run_xlat(torch, plan, x, None, n_out, 0)
    m = np.arange(n_out)
    hit = (m * D >= pos) & (m * D - (L - 1) <= pos)       # outputs whose window holds the NaN
    assert hit.sum() == 16
    assert np.all(np.isnan(y[hit].real) & np.isnan(y[hit].imag))
    assert not np.any(np.isnan(y[~hit]))
    clean = x.copy()
    clean[pos] = 0
    assert_tol(y[~hit], xlat_ref(clean, None, taps, D, plan.inc, 0, n_out)[~hit], "outputs outside the NaN's windows")
    plan.close()


def test_xlat_requires_hist_out(torch_cuda):
    torch = torch_cuda
    plan = nsh.FirXlatPlan(np.ones(4, np.float32), 2, 0.1)
    d = torch.zeros(64, dtype=torch.complex64, device="cuda")
    with pytest.raises(nsh.NshError, match="hist_out is required"):
        plan(d, None, None, d, 8, 0)
    plan.close()


# ---- timing: each entry point is exactly one launch ---------------------------------------------------
def test_armed_pair_taken_by_exactly_one_launch(torch_cuda, stream):
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

    n = 4099                                            # odd, and the pointers at 8 mod 16
    dx = dev(torch, stream[:n * 8 + 2])
    dy = torch.empty_like(dx)
    inc = nsh.phase_inc(0.1)
    count, rc, ms = timed(lambda: nsh.rotate_cc(dx.data_ptr() + 8, dy.data_ptr() + 8, n, inc, 3))
    assert count == 1 and rc == 0 and ms >= 0
    count, rc, ms = timed(lambda: nsh.rotate_cc(dx.data_ptr() + 8, dy.data_ptr(), n, inc, 3))  # 8-byte path
    assert count == 1 and rc == 0 and ms >= 0
    plan = nsh.FirXlatPlan(taps_for(127, 8), 8, 0.1)
    dh = torch.zeros(126, dtype=torch.complex64, device="cuda")
    count, rc, ms = timed(lambda: plan(dx.data_ptr() + 8, None, dh, dy, n, 0))
    assert count == 1 and rc == 0 and ms >= 0
    # n = 0: nothing launched, the pair dropped unrecorded
    count, rc, _ = timed(lambda: nsh.rotate_cc(dx, dy, 0, inc, 0))
    assert count == 0 and rc != 0
    count, rc, _ = timed(lambda: plan(dx, None, dh, dy, 0, 0))
    assert count == 0 and rc != 0
    plan.close()
