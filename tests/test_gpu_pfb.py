"""GPU: nsh_pfb_channelizer_ccf (k_pfb<M>) through the C-ABI.

Reference for every numeric check, computed here in numpy complex128 straight from the definition:
for each channel c, np.convolve(concat(hist, x), h * exp(2j pi ((c k) mod M) / M))[L-1::M][:n_out].
Judged with oracle.tol_ok (1e-5) on the whole (n_out, M) array jointly: the DFT mixes the channels,
so a quiet channel is accurate to the loudest one's level. Only the cross-check against
FirXlatPlan, on white input, compares single columns."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from newsched_amd import nsh
from tests.fir_accuracy import pfb_ref_conv as pfb_ref
from tests.gpu_util import assert_tol, dev, host, windowed_sinc

pytestmark = pytest.mark.gpu


def taps_for(L, M):
    return windowed_sinc(L, M)


@pytest.fixture(scope="module")
def stream():
    return orc.synth(1 << 17, 2024)


def run_pfb(torch, plan, x, hist, n_out, in_off=0, out_off=0):
    """One call; returns (y of shape (n_out, M), hist_out). hist None = NULL hist_in."""
    L, M = plan.ntaps, plan.nchans
    buf = np.zeros(n_out * M + 2, np.complex64)
    buf[in_off:in_off + n_out * M] = x[:n_out * M]
    dx = dev(torch, buf)
    dh = dev(torch, hist) if hist is not None and L > 1 else None
    dho = torch.full((max(L - 1, 1),), 5 + 5j, dtype=torch.complex64, device="cuda")
    dy = torch.full((n_out * M + 4,), 9 - 9j, dtype=torch.complex64, device="cuda")
    plan(dx.data_ptr() + 8 * in_off, dh, dho, dy.data_ptr() + 8 * out_off, n_out)
    y = host(dy)
    assert np.all(y[:out_off] == 9 - 9j) and np.all(y[out_off + n_out * M:] == 9 - 9j)  # nothing outside n_out * M
    return y[out_off:out_off + n_out * M].reshape(n_out, M), host(dho)[:L - 1]


CASES = [(2, 1, 1), (2, 64, 257), (4, 48, 1000), (8, 127, 2049), (16, 16, 5), (16, 127, 700), (32, 385, 300),
         (64, 65, 513), (64, 1024, 130)]


@pytest.mark.parametrize("case", CASES, ids=[f"M{m}-L{l}-n{n}" for m, l, n in CASES])
@pytest.mark.parametrize("with_hist", [True, False], ids=["hist", "nullhist"])
def test_pfb_cases(torch_cuda, stream, case, with_hist):
    torch = torch_cuda
    M, L, n_out = case
    taps = taps_for(L, M)
    plan = nsh.PfbPlan(taps, M)
    assert plan.kernel == f"k_pfb<{M}>" and plan.tile * M == 2048 and plan.ntaps == L and plan.nchans == M
    x = stream[2000:2000 + n_out * M]
    hist = stream[2000 - (L - 1):2000].copy() if with_hist else None
    y, ho = run_pfb(torch, plan, x, hist, n_out)
    assert_tol(y, pfb_ref(x, hist, taps, M, n_out), f"{plan.kernel} L={L}")
    raw = np.concatenate([hist if hist is not None else np.zeros(L - 1, np.complex64), x])
    np.testing.assert_array_equal(ho, raw[raw.size - (L - 1):])
    plan.close()


@pytest.mark.parametrize("M,L", [(2, 15), (4, 31), (8, 63), (16, 127), (32, 100), (64, 200)])
def test_pfb_tile_edges(torch_cuda, M, L):
    torch = torch_cuda
    taps = taps_for(L, M)
    plan = nsh.PfbPlan(taps, M)
    T = plan.tile
    x = orc.synth((3 * T + 1) * M + L - 1, 55)
    hist, x = x[:L - 1].copy(), x[L - 1:]
    ref = pfb_ref(x, hist, taps, M, 3 * T + 1)
    for n_out in (T - 1, T, T + 1, 3 * T + 1):
        y, _ = run_pfb(torch, plan, x, hist, n_out)
        assert_tol(y, ref[:n_out], f"{plan.kernel} T={T} n_out={n_out}")
    plan.close()


def test_pfb_chunked_stream_equals_one_call(torch_cuda, stream):
    torch = torch_cuda
    M, L = 8, 127
    taps = taps_for(L, M)
    plan = nsh.PfbPlan(taps, M)
    x = stream[:20000]
    whole, _ = run_pfb(torch, plan, x, None, 2500)
    out, hist, pos = [], None, 0
    for n_in in (8, 1240, 16, 7000, 20000 - 8264):
        y, hist = run_pfb(torch, plan, x[pos:pos + n_in], hist, n_in // M)
        out.append(y)
        pos += n_in
    assert pos == 20000
    y = np.concatenate(out)
    assert_tol(y, whole, "chunked vs one call")
    assert_tol(y, pfb_ref(x, None, taps, M, 2500), "chunked vs reference")
    plan.close()


@pytest.mark.parametrize("in_off,out_off", [(1, 0), (0, 1), (1, 1)])
def test_pfb_pointers_offset_by_8_bytes(torch_cuda, stream, in_off, out_off):
    torch = torch_cuda
    M, L, n_out = 16, 127, 700
    taps = taps_for(L, M)
    plan = nsh.PfbPlan(taps, M)
    x = stream[:n_out * M]
    hist = stream[-(L - 1):].copy()
    y, ho = run_pfb(torch, plan, x, hist, n_out, in_off=in_off, out_off=out_off)
    assert_tol(y, pfb_ref(x, hist, taps, M, n_out), f"in at {8 * in_off} mod 16, out at {8 * out_off} mod 16")
    np.testing.assert_array_equal(ho, x[-(L - 1):])
    plan.close()


@pytest.mark.parametrize("M,L", [(16, 127), (64, 200)])
def test_pfb_columns_equal_the_translating_fir(torch_cuda, stream, M, L):
    torch = torch_cuda
    n_out = 600
    taps = taps_for(L, M)
    plan = nsh.PfbPlan(taps, M)
    x = stream[5000:5000 + n_out * M]
    hist = stream[5000 - (L - 1):5000].copy()
    y, _ = run_pfb(torch, plan, x, hist, n_out)
    dx, dh = dev(torch, x), dev(torch, hist)
    for c in (0, 1, M // 2, M - 1):
        xl = nsh.FirXlatPlan(taps, M, c / M)
        dho = torch.empty(L - 1, dtype=torch.complex64, device="cuda")
        dy = torch.empty(n_out, dtype=torch.complex64, device="cuda")
        xl(dx, dh, dho, dy, n_out, 0)
        assert_tol(y[:, c], host(dy), f"M={M} column {c} vs {xl.kernel}", rel=2e-5)
        xl.close()
    plan.close()


def test_pfb_tone_lands_in_its_channel(torch_cuda):
    torch = torch_cuda
    M, L, n_out = 16, 127, 1000
    taps = taps_for(L, M)
    plan = nsh.PfbPlan(taps, M)
    n = np.arange(n_out * M)
    x = np.exp(2j * np.pi * (3 / 16 + 0.003) * n).astype(np.complex64)
    y, _ = run_pfb(torch, plan, x, None, n_out)
    level = np.abs(y[L // M + 1:]).mean(axis=0)       # past the filter's start-up
    print("  channel levels:", np.array2string(level, precision=4))
    assert level[3] > 0.9
    assert np.all(np.delete(level, 3) < 1e-2)
    assert_tol(y, pfb_ref(x, None, taps, M, n_out), "tone, judged jointly")
    plan.close()


@pytest.mark.parametrize("M,L,back", [(64, 65, 70), (8, 127, 3)])
def test_pfb_nan_reaches_exactly_its_windows(torch_cuda, stream, M, L, back):
    torch = torch_cuda
    n_out = 300
    taps = taps_for(L, M)
    plan = nsh.PfbPlan(taps, M)
    x = stream[:n_out * M].copy()
    pos = 100 * M - back          # (64, 65): 70 back from step 100 is past its 65 taps, inside the padding to 128
    x[pos] = np.nan
    y, _ = run_pfb(torch, plan, x, None, n_out)
    m = np.arange(n_out)
    hit = (m * M >= pos) & (m * M - (L - 1) <= pos)       # time steps whose L-tap window holds the NaN
    assert hit.sum() == ((L - 1 - (-pos) % M) // M + 1)
    if (M, L) == (64, 65):
        assert not hit[100] and hit[99] and hit.sum() == 1
    assert np.all(np.isnan(y[hit].real) & np.isnan(y[hit].imag))  # in all M channels
    assert not np.any(np.isnan(y[~hit]))
    clean = x.copy()
    clean[pos] = 0
    assert_tol(y[~hit], pfb_ref(clean, None, taps, M, n_out)[~hit], "time steps outside the NaN's windows")
    plan.close()


def test_pfb_requires_hist_out(torch_cuda):
    torch = torch_cuda
    plan = nsh.PfbPlan(np.ones(4, np.float32), 2)
    d = torch.zeros(64, dtype=torch.complex64, device="cuda")
    with pytest.raises(nsh.NshError, match="hist_out is required"):
        plan(d, None, None, d, 8)
    one = nsh.PfbPlan(np.ones(1, np.float32), 2)      # L = 1: no history at all
    dy = torch.zeros(64, dtype=torch.complex64, device="cuda")
    one(d, None, None, dy, 8)
    torch.cuda.synchronize()
    plan.close()
    one.close()


def test_pfb_armed_pair_taken_by_exactly_one_launch(torch_cuda, stream):
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

    n_out, M = 4099, 16
    dx = dev(torch, stream[:n_out * M + 2])
    dy = torch.empty_like(dx)
    plan = nsh.PfbPlan(taps_for(127, M), M)
    dh = torch.zeros(126, dtype=torch.complex64, device="cuda")
    count, rc, ms = timed(lambda: plan(dx.data_ptr() + 8, None, dh, dy, n_out))
    assert count == 1 and rc == 0 and ms >= 0
    count, rc, ms = timed(lambda: plan(dx, None, dh, dy.data_ptr() + 8, n_out))   # the 8-byte store path
    assert count == 1 and rc == 0 and ms >= 0
    count, rc, _ = timed(lambda: plan(dx, None, dh, dy, 0))   # nothing launched, the pair dropped unrecorded
    assert count == 0 and rc != 0
    plan.close()
