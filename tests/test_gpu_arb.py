"""GPU: nsh_arb_resamp_ccf (k_arb<R,P>) through the C-ABI.

Reference for every numeric check: arb_ref below, numpy complex128 straight from the definition (exact
integer phase in Python integers, the fp32 derivative taps d, mu as the kernel forms it), judged with
oracle.tol_ok at 1e-5. A numpy fp32 emulation of the kernel's order (arb_emulate_fp32: q ascending,
w = fl32(mu d + h), one rounding per multiply-add) stays within 3.6e-7 of it over CASES (worst at
F = 64, r = 64, 32 taps per output; 1.1e-7 to 2.5e-7 elsewhere; the single-tap case is exact), and within
the per-element bound everywhere, so the contract has a 28-fold margin for a correct fp32 kernel."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from newsched_amd import nsh
from tests.fir_accuracy import arb_indices, arb_ref, diff_taps
from tests.gpu_util import assert_tol, dev, host

pytestmark = pytest.mark.gpu

M31 = 2 ** 31 - 1


def windows(x, hist, taps, F, i, j):
    """Per q: (valid, tap index, index into [hist | x]) for the outputs at (i, j)."""
    L = len(taps); Q = -(-L // F); H = Q - 1
    h0 = np.zeros(H, x.dtype) if hist is None else hist
    ext = np.concatenate([h0, x])
    for q in range(Q):
        t = j + q * F
        yield t < L, np.minimum(t, L - 1), ext, i - q + H


def arb_emulate_fp32(x, hist, taps, F, step, phase, n_out):
    """The kernel's arithmetic in numpy: every multiply-add in double, rounded once to fp32."""
    i, j, mu = arb_indices(step, F, phase, n_out)
    h = np.asarray(taps, np.float32); d = diff_taps(taps)
    re = np.zeros(n_out, np.float32); im = np.zeros(n_out, np.float32)
    for valid, t, ext, xi in windows(x, hist, taps, F, i, j):
        xi = np.clip(xi, 0, ext.size - 1)
        w = (mu.astype(np.float64) * d[t] + h[t]).astype(np.float32).astype(np.float64)
        re = np.where(valid, (w * ext[xi].real + re).astype(np.float32), re)
        im = np.where(valid, (w * ext[xi].imag + im).astype(np.float32), im)
    return re + 1j * im


@pytest.fixture(scope="module")
def stream():
    return orc.synth(1 << 17, 2024)


def taps_for(L, F, rate):
    """Windowed sinc at F times the input rate, gain F, cut-off inside the narrower Nyquist band."""
    t = np.hamming(L) if L > 2 else np.ones(L)
    k = np.arange(L) - (L - 1) / 2.0
    t = t * np.sinc(0.8 * k / F * min(1.0, rate))
    return (F * t / t.sum()).astype(np.float32)


def inputs_for(plan, phase, n_out):
    """The fewest inputs that hold n_out outputs from phase: i(n_out - 1) + 1."""
    return (((phase + (n_out - 1) * plan.step) >> 32) // plan.nfilt) + 1 if n_out else 1


def run_arb(torch, plan, x, n_in, hist, n_out, phase=0, in_off=0, out_off=0, stream=None):
    """One call; returns (y, hist_out). hist None = NULL hist_in. Guard words around the output."""
    H = plan.history
    buf = np.zeros(n_in + 2, np.complex64)
    buf[in_off:in_off + n_in] = x[:n_in]
    dx = dev(torch, buf)
    dh = dev(torch, hist) if hist is not None and H > 0 else None
    dho = torch.full((max(H, 1),), 5 + 5j, dtype=torch.complex64, device="cuda")
    dy = torch.full((n_out + 6,), 9 - 9j, dtype=torch.complex64, device="cuda")
    o = 2 + out_off                                   # guard words before and after the output
    plan(dx.data_ptr() + 8 * in_off, n_in, dh, dho, dy.data_ptr() + 8 * o, n_out, phase, stream=stream)
    y = host(dy)
    assert np.all(y[:o] == 9 - 9j) and np.all(y[o + n_out:] == 9 - 9j)  # nothing outside n_out
    return y[o:o + n_out], host(dho)[:H]


def hist_after(x, hist, H, c):
    """The H raw samples before x[c]."""
    raw = np.concatenate([hist if hist is not None else np.zeros(H, np.complex64), x])
    return raw[c:c + H]


def instantiation(rate, F, L):
    Q = -(-L // F)
    step = round(F * 2 ** 32 / rate)
    if step <= F << 32:
        return "4,1"
    t_fit = ((8192 - Q) * (F << 32) - 1) // step + 1
    return "4,0" if t_fit >= 1024 else "2,0" if t_fit >= 512 else "1,0"


# (F, r, L, n_in): the issue's table; n_in keeps inputs and outputs below 2^17 and covers several tiles
CASES = [(2, 1.0, 1, 5000), (32, 160 / 147, 384, 30000), (32, 147 / 160, 400, 30000), (32, 1.0000001, 255, 20000),
         (16, 3.7, 100, 9000), (64, 64.0, 2048, 1500), (32, 1 / 64, 2048, 1 << 17), (64, 1 / 7.3, 1000, 60000),
         (8, np.pi / 3, 57, 20000)]


@pytest.mark.parametrize("case", CASES, ids=[f"F{f}-r{r:.7g}-L{l}" for f, r, l, n in CASES])
@pytest.mark.parametrize("with_hist", [True, False], ids=["hist", "nullhist"])
def test_arb_cases(torch_cuda, stream, case, with_hist):
    torch = torch_cuda
    F, rate, L, n_in = case
    taps = taps_for(L, F, rate)
    plan = nsh.ArbPlan(taps, rate, F)
    H = -(-L // F) - 1
    assert plan.kernel == f"k_arb<{instantiation(rate, F, L)}>" and plan.history == H
    assert (plan.ntaps, plan.nfilt) == (L, F) and plan.tile >= 110 and plan.tile % 2 == 0
    assert plan.step == nsh.arb_step(rate, F) and abs(plan.rate_effective / rate - 1) < 1e-9
    phase = 0 if not with_hist else (4 << 32) + 0x89abcdef      # the call starts between two inputs
    if H + n_in <= stream.size:
        before, x = stream[:H], stream[H:H + n_in]
    else:
        before, x = stream[stream.size - H:], stream[:n_in]
    hist = before.copy() if with_hist else None
    n_out, c, nxt = plan.span(phase, n_in, M31)
    assert c == n_in and n_out > 2 * plan.tile
    y, ho = run_arb(torch, plan, x, n_in, hist, n_out, phase)
    assert_tol(y, arb_ref(x, hist, taps, F, plan.step, phase, n_out), f"{plan.kernel} F={F} r={rate} L={L} n_out={n_out}")
    np.testing.assert_array_equal(ho, hist_after(x, hist, H, c))
    plan.close()


# one plan per instantiation
@pytest.mark.parametrize("F,rate,L", [(32, 160 / 147, 384), (64, 1 / 7.3, 1000), (32, 1 / 12, 200), (32, 1 / 64, 2048)])
def test_arb_tile_edges(torch_cuda, stream, F, rate, L):
    torch = torch_cuda
    taps = taps_for(L, F, rate)
    plan = nsh.ArbPlan(taps, rate, F)
    T, H = plan.tile, plan.history
    phase = 0x12345678
    n_all = inputs_for(plan, phase, 3 * T + 1)
    hist, x = stream[:H].copy(), stream[H:H + n_all]
    ref = arb_ref(x, hist, taps, F, plan.step, phase, 3 * T + 1)
    for n_out in (T - 1, T, T + 1, 3 * T + 1):
        n_in = inputs_for(plan, phase, n_out)             # the last window ends at the input's last sample
        assert plan.span(phase, n_in, M31)[0] >= n_out > plan.span(phase, n_in - 1, M31)[0]
        y, ho = run_arb(torch, plan, x, n_in, hist, n_out, phase)
        assert_tol(y, ref[:n_out], f"{plan.kernel} tile={T} n_out={n_out}")
        np.testing.assert_array_equal(ho, hist_after(x, hist, H, plan.span(phase, n_in, n_out)[1]))
    plan.close()


@pytest.mark.parametrize("F,rate,L", [(32, 160 / 147, 384), (32, 147 / 160, 400)])
@pytest.mark.parametrize("in_off,out_off", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_arb_pointers_offset_by_8_bytes(torch_cuda, stream, F, rate, L, in_off, out_off):
    torch = torch_cuda
    n_in = 3001
    taps = taps_for(L, F, rate)
    plan = nsh.ArbPlan(taps, rate, F)
    H = plan.history
    x = stream[:n_in]
    hist = stream[-H:].copy()
    n_out, c, _ = plan.span(0, n_in, M31)
    y, ho = run_arb(torch, plan, x, n_in, hist, n_out, 0, in_off=in_off, out_off=out_off)
    assert_tol(y, arb_ref(x, hist, taps, F, plan.step, 0, n_out), f"in at {8 * in_off} mod 16, out at {8 * out_off} mod 16")
    np.testing.assert_array_equal(ho, x[-H:])
    plan.close()


@pytest.mark.parametrize("F,rate,L", [(32, 160 / 147, 384), (32, 147 / 160, 400), (16, 3.7, 100), (64, 1 / 7.3, 1000),
                                      (32, 1 / 64, 2048), (2, 1.0, 1)])
def test_arb_chunked_stream_is_bit_identical(torch_cuda, stream, F, rate, L):
    """Random cuts, phase and history chained, some calls wanting fewer outputs than they hold and some
    holding none (advancing calls): the same bits as one call."""
    torch = torch_cuda
    taps = taps_for(L, F, rate)
    plan = nsh.ArbPlan(taps, rate, F)
    T, H = plan.tile, plan.history
    n_in = min(inputs_for(plan, 0, 2 * T + 50), 1 << 16)
    x = stream[:n_in]
    total, c_all, nxt_all = plan.span(0, n_in, M31)
    whole, hw = run_arb(torch, plan, x, n_in, None, total)
    rng = np.random.default_rng(int(F * 1000 + L))
    out, hist, pos, phase, advancing = [], None, 0, 0, 0
    while pos < n_in:
        n = int(min(rng.choice([1, 2, 7, 40, 300, 5000]), n_in - pos))
        want = int(rng.choice([0, 1, 33, M31, M31, M31]))
        n_out, c, nxt = plan.span(phase, n, want)
        advancing += n_out == 0 and c > 0
        y, hist = run_arb(torch, plan, x[pos:], n, hist, n_out, phase, out_off=len(out) & 1)
        out.append(y)
        pos, phase = pos + c, nxt
    y = np.concatenate(out)
    assert pos == c_all == n_in and phase == nxt_all and y.size == total
    np.testing.assert_array_equal(y.view(np.uint32), whole.view(np.uint32))
    np.testing.assert_array_equal(hist, hw)
    print(f"  {plan.kernel}: {len(out)} calls, {advancing} advancing")
    assert_tol(y, arb_ref(x, None, taps, F, plan.step, 0, total), "chunked vs reference")
    plan.close()


def test_arb_advancing_call_leaves_out_untouched(torch_cuda, stream):
    torch = torch_cuda
    F, rate, L = 32, 1 / 64, 2048
    plan = nsh.ArbPlan(taps_for(L, F, rate), rate, F)
    H = plan.history
    assert H == 63
    hist, x = stream[:H].copy(), stream[H:H + 40]
    phase = (50 * F) << 32                                   # the next output lies 50 inputs ahead
    for n_in in (1, 17, 40):
        assert plan.span(phase, n_in, M31) == (0, n_in, phase - ((n_in * F) << 32))
        y, ho = run_arb(torch, plan, x, n_in, hist, 0, phase)     # run_arb checks that out keeps its guard words
        assert y.size == 0
        np.testing.assert_array_equal(ho, hist_after(x, hist, H, n_in))
        _, ho = run_arb(torch, plan, x, n_in, None, 0, phase)     # NULL hist_in: zeros move in
        np.testing.assert_array_equal(ho, hist_after(x, None, H, n_in))
    one = nsh.ArbPlan(np.ones(2, np.float32), rate, 2)            # Q = 1: no history, nothing to launch
    assert one.history == 0
    y, _ = run_arb(torch, one, x, 5, None, 0, (50 * 2) << 32)
    plan.close()
    one.close()


def test_arb_integer_step_equals_the_rational_resampler(torch_cuda, stream):
    """r = 32/21 with F = 32: the step is 21 whole filter steps, mu is 0, and output n is
    nsh_resamp_ccf(I = 32, D = 21)'s on the same taps."""
    torch = torch_cuda
    F, D, L, n_units = 32, 21, 384, 700
    taps = taps_for(L, F, 32 / 21)
    plan = nsh.ArbPlan(taps, 32 / 21, F)
    assert plan.step == D << 32
    rs = nsh.ResampPlan(taps, F, D)
    assert rs.history == plan.history
    H = plan.history
    hist, x = stream[:H].copy(), stream[H:H + n_units * D]
    n_in, n_out = n_units * D, n_units * F
    assert plan.span(0, n_in, M31) == (n_out, n_in, 0)
    y, ho = run_arb(torch, plan, x, n_in, hist, n_out)
    dho = torch.empty(max(H, 1), dtype=torch.complex64, device="cuda")
    dy = torch.empty(n_out, dtype=torch.complex64, device="cuda")
    rs(dev(torch, x), dev(torch, hist), dho, dy, n_units)
    yr = host(dy)
    assert_tol(y, yr, f"{plan.kernel} vs {rs.kernel}")
    print("  bit-identical to nsh_resamp_ccf:", bool(np.array_equal(y.view(np.uint32), yr.view(np.uint32))))
    np.testing.assert_array_equal(ho, host(dho)[:H])
    assert_tol(y, arb_ref(x, hist, taps, F, plan.step, 0, n_out), "vs reference")
    rs.close()
    plan.close()


# (16, 3.7, 100): L is no multiple of F, filters 4 .. 15 have one tap fewer than Q = 7
@pytest.mark.parametrize("F,rate,L", [(16, 3.7, 100), (32, 147 / 160, 400), (64, 1 / 7.3, 1000), (8, np.pi / 3, 57)])
@pytest.mark.parametrize("spike", [complex(np.nan, np.nan), complex(np.inf, 0)], ids=["nan", "inf"])
def test_arb_non_finite_reaches_exactly_its_outputs(torch_cuda, stream, F, rate, L, spike):
    torch = torch_cuda
    n_in = 4000
    taps = taps_for(L, F, rate)
    plan = nsh.ArbPlan(taps, rate, F)
    x = stream[:n_in].copy()
    n_out = plan.span(0, n_in, M31)[0]
    clean, _ = run_arb(torch, plan, x, n_in, None, n_out)
    s = 1501
    x[s] = spike
    y, _ = run_arb(torch, plan, x, n_in, None, n_out)
    i, j, mu = arb_indices(plan.step, F, 0, n_out)
    q = i - s                                            # the tap row that meets sample s in output n
    hit = (q >= 0) & (j + q * F < L)
    # an inf sample times a zero coefficient is NaN: non-finite either way; no coefficient h + mu d is
    # relied on to be non-zero
    assert 0 < hit.sum() < n_out
    bad = ~(np.isfinite(y.real) & np.isfinite(y.imag))
    np.testing.assert_array_equal(bad, hit)
    np.testing.assert_array_equal(y[~hit].view(np.uint32), clean[~hit].view(np.uint32))
    plan.close()


def test_arb_refusals_that_need_a_plan(torch_cuda):
    torch = torch_cuda
    plan = nsh.ArbPlan(np.ones(8, np.float32), 1.5, 4)         # Q = 2
    d = torch.zeros(64, dtype=torch.complex64, device="cuda")
    dy = torch.full((200,), 9 - 9j, dtype=torch.complex64, device="cuda")
    dh = torch.zeros(4, dtype=torch.complex64, device="cuda")
    with pytest.raises(nsh.NshError, match="hist_out is required"):
        plan(d, 32, None, None, dy, 8)
    most = plan.span(0, 32, M31)[0]
    with pytest.raises(nsh.NshError, match="n_out is more than n_in inputs hold"):
        plan(d, 32, None, dh, dy, most + 1)
    with pytest.raises(nsh.NshError, match="n_out is more than n_in inputs hold"):
        plan(d, 32, None, dh, dy, 1, phase=(32 * 4) << 32)
    assert np.all(host(dy) == 9 - 9j)
    plan(d, 32, None, dh, dy, most)
    plan(d, 0, None, dh, dy, 0)                                # n_in = 0: nothing
    torch.cuda.synchronize()
    one = nsh.ArbPlan(np.ones(2, np.float32), 1.5, 2)          # Q = 1: no history at all
    assert one.history == 0
    one(d, 32, None, None, dy, one.span(0, 32, M31)[0])
    torch.cuda.synchronize()
    plan.close()
    one.close()


def test_arb_two_streams_give_the_same_bits(torch_cuda, stream):
    torch = torch_cuda
    F, rate, L, n_in = 32, 160 / 147, 384, 9000
    plan = nsh.ArbPlan(taps_for(L, F, rate), rate, F)
    x = stream[:n_in]
    n_out = plan.span(0, n_in, M31)[0]
    ya, _ = run_arb(torch, plan, x, n_in, None, n_out)
    s = torch.cuda.Stream()
    yb, _ = run_arb(torch, plan, x, n_in, None, n_out, stream=s)
    np.testing.assert_array_equal(ya.view(np.uint32), yb.view(np.uint32))
    plan.close()


def test_arb_armed_pair_taken_by_exactly_one_launch(torch_cuda, stream):
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

    F, rate, n_in = 32, 147 / 160, 5000
    plan = nsh.ArbPlan(taps_for(400, F, rate), rate, F)
    n_out = plan.span(0, n_in, M31)[0]
    dx = dev(torch, stream[:n_in + 2])
    dy = torch.full((n_out + 2,), 9 - 9j, dtype=torch.complex64, device="cuda")
    dh = torch.zeros(max(plan.history, 1), dtype=torch.complex64, device="cuda")
    count, rc, ms = timed(lambda: plan(dx.data_ptr() + 8, n_in, None, dh, dy, n_out))
    assert count == 1 and rc == 0 and ms >= 0
    count, rc, ms = timed(lambda: plan(dx, n_in, None, dh, dy.data_ptr() + 8, n_out))   # the 8-byte store path
    assert count == 1 and rc == 0 and ms >= 0
    count, rc, ms = timed(lambda: plan(dx, 3, None, dh, dy, 0, phase=(F * 9) << 32))     # an advancing call is a launch
    assert count == 1 and rc == 0 and ms >= 0
    dy.fill_(9 - 9j)
    count, rc, _ = timed(lambda: plan(dx, 0, None, dh, dy, 0))   # no input: nothing launched, the pair dropped unrecorded
    assert count == 0 and rc != 0
    assert np.all(host(dy) == 9 - 9j)
    plan.close()
