"""GPU: nsh_pfb_synthesizer_ccf (k_pfb_synth<M>) through the C-ABI.

Reference for every numeric check: fir_accuracy.synth_ref (ref_of here), the polyphase model in numpy complex128 (an
unnormalised inverse DFT across the channels of every item, then the M branch FIRs). Judged with
oracle.tol_ok (1e-5) on the whole output jointly: the DFT mixes the channels, so the accuracy is
relative to the loudest. Every case also checks that nothing outside the n_in * M outputs is written
and that hist_out holds the last Q-1 raw items bit for bit."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from newsched_amd import nsh
from tests.fir_accuracy import synth_ref as ref_of
from tests.gpu_util import assert_tol, dev, host, windowed_sinc

pytestmark = pytest.mark.gpu


def taps_for(L, M):
    return windowed_sinc(L, M)


@pytest.fixture(scope="module")
def stream():
    return orc.synth(1 << 17, 2025)


def run_synth(torch, plan, x, hist, n_in, in_off=0, out_off=0):
    """One call on n_in items of x (flat); returns (y of n_in * M samples, hist_out). hist None = NULL hist_in."""
    M = plan.nchans
    H = (-(-plan.ntaps // M) - 1) * M
    buf = np.zeros(n_in * M + 2, np.complex64)
    buf[in_off:in_off + n_in * M] = x[:n_in * M]
    dx = dev(torch, buf)
    dh = dev(torch, hist) if hist is not None and H > 0 else None
    dho = torch.full((max(H, 1),), 5 + 5j, dtype=torch.complex64, device="cuda")
    dy = torch.full((n_in * M + 4,), 9 - 9j, dtype=torch.complex64, device="cuda")
    plan(dx.data_ptr() + 8 * in_off, dh, dho, dy.data_ptr() + 8 * out_off, n_in)
    y = host(dy)
    assert np.all(y[:out_off] == 9 - 9j) and np.all(y[out_off + n_in * M:] == 9 - 9j)  # nothing outside n_in * M
    ho = host(dho)
    if H == 0:
        assert ho[0] == 5 + 5j
    return y[out_off:out_off + n_in * M], ho[:H]


def check_hist(ho, hist, x, H):
    raw = np.concatenate([hist if hist is not None else np.zeros(H, np.complex64), x])
    np.testing.assert_array_equal(ho, raw[raw.size - H:])


CASES = [(2, 1, 1), (2, 64, 257), (4, 48, 1000), (8, 127, 2049), (16, 16, 5), (16, 127, 700), (32, 385, 300),
         (64, 65, 513), (64, 1024, 130)]


@pytest.mark.parametrize("case", CASES, ids=[f"M{m}-L{l}-n{n}" for m, l, n in CASES])
@pytest.mark.parametrize("with_hist", [True, False], ids=["hist", "nullhist"])
def test_synth_cases(torch_cuda, stream, case, with_hist):
    torch = torch_cuda
    M, L, n_in = case
    H = (-(-L // M) - 1) * M
    taps = taps_for(L, M)
    plan = nsh.PfbSynthPlan(taps, M)
    assert plan.kernel == f"k_pfb_synth<{M}>" and plan.tile * M == 2048 and plan.ntaps == L and plan.nchans == M
    x = stream[2048:2048 + n_in * M]
    hist = stream[2048 - H:2048].copy() if with_hist else None
    y, ho = run_synth(torch, plan, x, hist, n_in)
    assert_tol(y, ref_of(x, hist, taps, M), f"{plan.kernel} L={L}")
    check_hist(ho, hist, x, H)
    plan.close()


@pytest.mark.parametrize("M,L", [(2, 15), (4, 31), (8, 63), (16, 127), (32, 100), (64, 200)])
def test_synth_tile_edges(torch_cuda, M, L):
    torch = torch_cuda
    H = (-(-L // M) - 1) * M
    taps = taps_for(L, M)
    plan = nsh.PfbSynthPlan(taps, M)
    T = plan.tile
    x = orc.synth((3 * T + 1) * M + H, 56)
    hist, x = x[:H].copy(), x[H:]
    ref = ref_of(x, hist, taps, M)
    for n_in in (T - 1, T, T + 1, 3 * T + 1):
        y, ho = run_synth(torch, plan, x, hist, n_in)
        assert_tol(y, ref[:n_in * M], f"{plan.kernel} T={T} n_in={n_in}")
        check_hist(ho, hist, x[:n_in * M], H)
    plan.close()


def test_synth_chunked_stream_equals_one_call(torch_cuda, stream):
    torch = torch_cuda
    M, L, n = 8, 127, 2500
    H = (-(-L // M) - 1) * M
    taps = taps_for(L, M)
    plan = nsh.PfbSynthPlan(taps, M)
    x = stream[:n * M]
    whole, _ = run_synth(torch, plan, x, None, n)
    out, hist, pos = [], None, 0
    for n_in in (1, 155, 2, 875, n - 1033):
        y, hist = run_synth(torch, plan, x[pos * M:(pos + n_in) * M], hist, n_in)
        out.append(y)
        pos += n_in
    assert pos == n
    y = np.concatenate(out)
    assert_tol(y, whole, "chunked vs one call")
    assert_tol(y, ref_of(x, None, taps, M), "chunked vs reference")
    np.testing.assert_array_equal(hist, x[x.size - H:])
    plan.close()


@pytest.mark.parametrize("in_off,out_off", [(1, 0), (0, 1), (1, 1)])
def test_synth_pointers_offset_by_8_bytes(torch_cuda, stream, in_off, out_off):
    torch = torch_cuda
    M, L, n_in = 16, 127, 700
    H = (-(-L // M) - 1) * M
    taps = taps_for(L, M)
    plan = nsh.PfbSynthPlan(taps, M)
    x = stream[:n_in * M]
    hist = stream[-H:].copy()
    y, ho = run_synth(torch, plan, x, hist, n_in, in_off=in_off, out_off=out_off)
    assert_tol(y, ref_of(x, hist, taps, M), f"in at {8 * in_off} mod 16, out at {8 * out_off} mod 16")
    np.testing.assert_array_equal(ho, x[-H:])
    plan.close()


@pytest.mark.parametrize("M,L", [(16, 127), (64, 200)])
def test_synth_equals_the_sum_of_rotated_interpolators(torch_cuda, stream, M, L):
    """y = sum_c rot_c(ResampPlan(I = M, D = 1, taps)(X[:, c])): the resampler on the GPU, the rotation by
    exp(2j pi c n / M) and the sum in float64 on the host."""
    torch = torch_cuda
    n_in = 300
    taps = taps_for(L, M)
    plan = nsh.PfbSynthPlan(taps, M)
    x = stream[7000:7000 + n_in * M]
    y, _ = run_synth(torch, plan, x, None, n_in)
    rs = nsh.ResampPlan(taps, M, 1)
    n = np.arange(n_in * M)
    acc = np.zeros(n_in * M, np.complex128)
    dho = torch.empty(max(rs.history, 1), dtype=torch.complex64, device="cuda")
    for c in range(M):
        dy = torch.empty(n_in * M, dtype=torch.complex64, device="cuda")
        rs(dev(torch, x.reshape(n_in, M)[:, c]), None, dho, dy, n_in)
        acc += host(dy).astype(np.complex128) * np.exp(2j * np.pi * ((c * n) % M) / M)
    assert_tol(y, acc, f"M={M} vs {M} x {rs.kernel}, rotated and summed", rel=2e-5)
    rs.close()
    plan.close()


def test_synth_tone_lands_at_its_frequency(torch_cuda):
    torch = torch_cuda
    M, L, n_in = 16, 127, 300
    taps = (M * taps_for(L, M)).astype(np.float32)
    plan = nsh.PfbSynthPlan(taps, M)
    X = np.zeros((n_in, M), np.complex64)
    X[:, 3] = 1
    y, _ = run_synth(torch, plan, X.reshape(-1), None, n_in)
    assert_tol(y, ref_of(X.reshape(-1), None, taps, M), "tone")
    spec = np.abs(np.fft.fft(y[L:L + 4096].astype(np.complex128))) / 4096       # past the filter's start-up
    peak = int(np.argmax(spec))
    rest = np.delete(spec, peak).max()
    print(f"  peak bin {peak} at level {spec[peak]:.6f}, next-largest bin {rest:.3g}")
    assert peak == 768 and abs(spec[peak] - 1.0) < 1e-3
    assert rest < 1e-2


@pytest.mark.parametrize("M", [4, 16, 64])
def test_synth_then_channelizer_round_trip(torch_cuda, M):
    """Synthesizer (taps M h) into PfbPlan (taps h), L = 8 M + 1: the channelizer's output, delayed by
    exactly 8 items, is the input to the prototype's passband error (5.9e-3 to 6.5e-3 in float64; a
    delay off by one item gives at least 9.8e-2)."""
    torch = torch_cuda
    L, n_in = 8 * M + 1, 200
    h = taps_for(L, M)
    m = np.arange(n_in)[:, None]
    c = np.arange(M)[None, :]
    X = ((c + 1) / M * np.exp(2j * np.pi * ((7 * c) % 5 - 2) * 0.01 * m)).astype(np.complex64)
    syn = nsh.PfbSynthPlan((M * h).astype(np.float32), M)
    y, _ = run_synth(torch, syn, X.reshape(-1), None, n_in)
    ana = nsh.PfbPlan(h, M)
    dho = torch.empty(L - 1, dtype=torch.complex64, device="cuda")
    dz = torch.empty(n_in * M, dtype=torch.complex64, device="cuda")
    ana(dev(torch, y), None, dho, dz, n_in)
    Z = host(dz).reshape(n_in, M)
    err = np.abs(Z[18:] - X[18 - 8:n_in - 8]).max()
    off = min(np.abs(Z[18:] - X[18 - d:n_in - d]).max() for d in (7, 9))
    print(f"  M={M}: round-trip max error {err:.3g} (delay off by one item: {off:.3g})")
    assert err < 2e-2
    syn.close()
    ana.close()


@pytest.mark.parametrize("M,L", [(64, 65), (8, 127)])
def test_synth_nan_reaches_exactly_its_outputs(torch_cuda, stream, M, L):
    torch = torch_cuda
    n_in = 300
    taps = taps_for(L, M)
    plan = nsh.PfbSynthPlan(taps, M)
    x = stream[:n_in * M].copy()
    x[100 * M + M // 3] = np.nan
    y, _ = run_synth(torch, plan, x, None, n_in)
    hit = np.zeros(n_in * M, bool)
    hit[100 * M:100 * M + L] = True
    assert np.all(np.isnan(y[hit].real) & np.isnan(y[hit].imag))
    assert not np.any(np.isnan(y[~hit]))
    clean = x.copy()
    clean[100 * M + M // 3] = 0
    assert_tol(y[~hit], ref_of(clean, None, taps, M)[~hit], "outputs outside the NaN's reach")
    plan.close()


def test_synth_requires_hist_out(torch_cuda):
    torch = torch_cuda
    plan = nsh.PfbSynthPlan(np.ones(4, np.float32), 2)
    d = torch.zeros(64, dtype=torch.complex64, device="cuda")
    with pytest.raises(nsh.NshError, match="hist_out is required"):
        plan(d, None, None, d, 8)
    one = nsh.PfbSynthPlan(np.ones(2, np.float32), 2)      # L <= M: no history at all
    dx = dev(torch, np.arange(16, dtype=np.float32).astype(np.complex64))
    dy = torch.zeros(64, dtype=torch.complex64, device="cuda")
    one(dx, None, None, dy, 8)
    X = np.arange(16.0).reshape(8, 2)
    np.testing.assert_array_equal(host(dy)[:16], np.stack([X[:, 0] + X[:, 1], X[:, 0] - X[:, 1]], 1).reshape(-1))
    plan.close()
    one.close()


def test_synth_armed_pair_taken_by_exactly_one_launch(torch_cuda, stream):
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

    n_in, M = 259, 16
    dx = dev(torch, stream[:n_in * M + 2])
    dy = torch.empty_like(dx)
    plan = nsh.PfbSynthPlan(taps_for(127, M), M)
    dh = torch.zeros(7 * M, dtype=torch.complex64, device="cuda")
    count, rc, ms = timed(lambda: plan(dx.data_ptr() + 8, None, dh, dy, n_in))   # the 16-byte store path
    assert count == 1 and rc == 0 and ms >= 0
    count, rc, ms = timed(lambda: plan(dx, None, dh, dy.data_ptr() + 8, n_in))   # the 8-byte store path
    assert count == 1 and rc == 0 and ms >= 0
    count, rc, _ = timed(lambda: plan(dx, None, dh, dy, 0))   # nothing launched, the pair dropped unrecorded
    assert count == 0 and rc != 0
    plan.close()
