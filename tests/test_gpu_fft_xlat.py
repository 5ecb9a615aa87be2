"""GPU: nsh_fft_xlat_ccc (k_fft_xlat<N, D>: tune, overlap-save FIR with complex taps, decimate) in all
28 (N, D) forms.

Reference (float64, tests/fft_xlat_ref.py, checked against a term-by-term sum in
tests/test_fft_xlat_abi.py): every sample of hist_in ++ in rotated by its own 64-bit phase, convolved
with the taps in complex128, every D-th output. The header's bound, per output m of frame f = m // Vd:
    |y - y_ref| <= 1e-5 |y_ref| + 1e-6 * max|x over frame f's window| * sum_k |h[k]|
asserted per output. Every form prints its worst err / bound beside the same ratio of the kernel's
chain in numpy / scipy complex64 on the same frames (model_c64: reported here, asserted in
tests/test_gpu_fft_accuracy.py, which holds all 28 forms to the model's rms error, tuned and untuned).
hist_out is bit-exact in every test that runs the kernel, and two guard samples on each side of out
and hist_out stay untouched.

Shapes: at most 2 tile + 1 frames (about 9 N samples at N = 1024): one partial frame, exactly tile
frames, tile + 1 frames, and 2 tile + 1 under a grid cap of 1 (the second loop trip, which runs on the
prefetched window).

Measured on one MI355X (worst err / bound over this file): 0.17 (impulse tap at delay 4095, N = 8192,
D = 4); 0.029 to 0.088 over the 28 forms beside 0.027 to 0.090 for the complex64 model; DESIGN.md
section 4.10."""
import ctypes as C

import numpy as np
import pytest

from newsched_amd import nsh
from tests.gpu_util import bits, uniform
from tests import fft_xlat_ref as ref

pytestmark = pytest.mark.gpu

SIZES, DECIMS = ref.SIZES, ref.DECIMS
GUARD = complex(123.0, -77.0)
NG = 2  # guard samples on each side of out and hist_out
FREQ = 0.1137
sizes = pytest.mark.parametrize("N", SIZES)


def tone(n, inc, first=0, lo=0):
    """exp(-j 2 pi phase(first + i)), i in [lo, lo + n): the signal that the block's rotation turns
    into the constant 1."""
    return np.exp(-2j * np.pi * ref.turns(first, lo, lo + n, inc))


def signal(n, inc, seed):
    """Noise plus a tone at center_freq."""
    return (0.5 * uniform(n, seed) + 0.5 * tone(n, inc)).astype(np.complex64)


def lowpass(L, D):
    import scipy.signal as ss

    return ss.firwin(L, 0.8 / D if D > 1 else 0.4).astype(np.complex64)


def run(torch, plan, x, hist=None, first=0, odd=0, want_hist=True):
    """One call over x (len(x) // D outputs) with every pointer `odd` samples (8 bytes each) into its
    allocation, NG guard samples on each side of out and hist_out; checks the guards and hist_out's
    bits; returns out."""
    D, H = plan.decim, plan.hist_len
    n_out = len(x) // D
    n = n_out * D
    dx = torch.zeros(odd + n, dtype=torch.complex64, device="cuda")
    dx[odd:] = torch.from_numpy(np.array(x[:n], np.complex64)).cuda()
    dy = torch.full((odd + NG + n_out + NG,), GUARD, dtype=torch.complex64, device="cuda")
    dho = torch.full((odd + NG + H + NG,), GUARD, dtype=torch.complex64, device="cuda")
    dhi = None
    if hist is not None:
        dhi = torch.zeros(odd + H, dtype=torch.complex64, device="cuda")
        dhi[odd:] = torch.from_numpy(np.array(hist, np.complex64)).cuda()
    plan(dx.data_ptr() + 8 * odd, None if dhi is None else dhi.data_ptr() + 8 * odd,
         dho.data_ptr() + 8 * (odd + NG) if (H or want_hist) else None, dy.data_ptr() + 8 * (odd + NG), n_out, first)
    torch.cuda.synchronize()
    y, ho = dy.cpu().numpy(), dho.cpu().numpy()
    g = np.complex64(GUARD)
    assert np.all(y[:odd + NG] == g) and np.all(y[odd + NG + n_out:] == g), (plan.kernel, n_out, odd)
    assert np.all(ho[:odd + NG] == g) and np.all(ho[odd + NG + H:] == g), (plan.kernel, n_out, odd)
    tail = np.concatenate([np.zeros(H, np.complex64) if hist is None else np.asarray(hist, np.complex64),
                           np.asarray(x[:n], np.complex64)])[n:]
    assert np.array_equal(bits(ho[odd + NG:odd + NG + H], np.complex64), bits(tail, np.complex64)), (plan.kernel, n_out, "hist_out")
    return y[odd + NG:odd + NG + n_out]


def check(name, plan, x, h, y, hist=None, first=0, printed=False):
    N, D = plan.fft_size, plan.decim
    r = ref.ref64(x, h, D, plan.phase_inc, first, hist)
    b = ref.bound(x, h, D, N, r, hist)
    w = ref.worst(y, r, b)
    if printed:
        wm = ref.worst(ref.model_c64(x, h, D, N, plan.phase_inc, first, hist), r, b)
        print(f"{name} {plan.kernel} L={len(h)} n_out={len(y)}: worst err/bound {w:.4f}, complex64 model {wm:.4f}")
    assert w <= 1.0, (name, plan.kernel, len(h), len(y), w)
    return w


def frames_len(plan, frames, extra=0):
    """Inputs of a call of `frames` whole frames plus `extra` outputs."""
    return (frames * plan.valid // plan.decim + extra) * plan.decim


# ---- a. every form on the shapes that reach every path ----------------------------------------------
@sizes
@pytest.mark.parametrize("D", DECIMS)
def test_every_form(torch_cuda, N, D):
    L = 128  # L - 1 odd: no multiple of any D > 1
    h = lowpass(L, D)
    p = nsh.FftXlatPlan(h, D, FREQ, fft_size=N)
    Nm, O, V = ref.geometry(L, D, N)
    assert (p.fft_size, p.overlap, p.valid, p.kernel) == (N, O, V, f"k_fft_xlat<{N}, {D}>")
    assert O > L - 1 or D == 1
    tile, Vd = p.tile, V // D
    x = signal(frames_len(p, 2 * tile + 1), p.phase_inc, N + D)
    hist = uniform(L - 1, 7)
    w = 0.0
    for n_out in (Vd // 2 + 1, tile * Vd, tile * Vd + 3):
        xi = x[:n_out * D]
        w = max(w, check("form", p, xi, h, run(torch_cuda, p, xi, hist, first=12345), hist, 12345))
    p.grid_cap(1)
    y = run(torch_cuda, p, x, hist, first=12345)
    w = max(w, check("form, cap 1", p, x, h, y, hist, 12345, printed=True))
    print(f"every form {p.kernel}: worst err/bound {w:.4f}")
    p.close()


@sizes
@pytest.mark.parametrize("Lk", ["1", "N/2"])
def test_shortest_and_longest_taps(torch_cuda, N, Lk):
    L, D = (1, 8) if Lk == "1" else (N // 2, 4)
    h = uniform(L, 1000 + L) * np.float32(1.0 if L == 1 else 0.05)
    p = nsh.FftXlatPlan(h, D, -FREQ, fft_size=N)
    assert p.overlap == (0 if L == 1 else N // 2)
    x = signal(frames_len(p, p.tile + 1, 5), p.phase_inc, 3 * N)
    check("taps " + Lk, p, x, h, run(torch_cuda, p, x, first=99, want_hist=False), None, 99, printed=True)
    p.close()


# ---- b. what the definition pins ---------------------------------------------------------------------
@sizes
def test_decimation_one_untuned_is_fft_filter_bit_for_bit(torch_cuda, N):
    torch = torch_cuda
    h = uniform(127, 5)
    p = nsh.FftXlatPlan(h, 1, 0.0, fft_size=N)
    q = nsh.FftFilterPlan(h, N)
    assert p.phase_inc == 0 and p.valid == q.valid
    x = uniform(frames_len(p, 2 * p.tile + 1, 7), N)
    hist = uniform(126, 6)
    y = run(torch, p, x, hist)
    dx, dh = torch.from_numpy(x).cuda(), torch.from_numpy(hist).cuda()
    dy, dho = torch.empty_like(dx), torch.empty_like(dh)
    q(dx, dh, dho, dy, len(x))
    torch.cuda.synchronize()
    assert np.array_equal(bits(y, np.complex64), bits(dy.cpu().numpy(), np.complex64))
    p.close()
    q.close()


@pytest.mark.parametrize("N,D", [(1024, 4), (4096, 16), (8192, 2)])
def test_untuned_is_every_dth_output_of_fft_filter(torch_cuda, N, D):
    torch = torch_cuda
    L = 130
    h = uniform(L, 8)
    p = nsh.FftXlatPlan(h, D, 0.0, fft_size=N)
    q = nsh.FftFilterPlan(h, N)
    x = uniform(frames_len(p, p.tile + 1, 3), N + D)
    y = run(torch, p, x)
    dx = torch.from_numpy(x).cuda()
    dy, dho = torch.empty_like(dx), torch.empty(L - 1, dtype=torch.complex64, device="cuda")
    q(dx, None, dho, dy, len(x))
    torch.cuda.synchronize()
    yf = dy.cpu().numpy()[::D]
    r = ref.ref64(x, h, D, 0)
    # fft_filter_ccc's own bound at these outputs: its frames' windows
    V1 = N - (L - 1)
    s = np.abs(np.concatenate([np.zeros(L - 1), x, np.zeros(N + V1)]))
    w1 = np.array([s[f * V1:f * V1 + N].max() for f in range(-(-len(x) // V1))])
    b1 = (1e-5 * np.abs(r) + 1e-6 * np.repeat(w1, V1)[:len(x)][::D] * np.abs(h.astype(np.complex128)).sum())
    b = ref.bound(x, h, D, N, r) + b1
    e = np.abs(y.astype(np.complex128) - yf.astype(np.complex128))
    print(f"{p.kernel} against {q.kernel}[::{D}]: worst difference / (sum of both bounds) {np.max(e / b):.4f}")
    assert np.all(e <= b)
    p.close()
    q.close()


@pytest.mark.parametrize("D,L", [(1, 127), (2, 127), (8, 128), (16, 255), (64, 1024)])
def test_real_taps_agree_with_the_fused_fir(torch_cuda, D, L):
    torch = torch_cuda
    import scipy.signal as ss

    hr = ss.firwin(L, 0.8 / max(D, 2)).astype(np.float32)
    h = hr.astype(np.complex64)
    first = (1 << 40) + 3
    p = nsh.FftXlatPlan(h, D, FREQ)
    q = nsh.FirXlatPlan(hr, D, FREQ)
    assert p.phase_inc == q.inc
    x = signal(frames_len(p, p.tile + 1, 3), p.phase_inc, D + L)
    hist = uniform(L - 1, 9)
    y = run(torch, p, x, hist, first)
    n_out = len(x) // D
    dx, dh = torch.from_numpy(x).cuda(), torch.from_numpy(hist).cuda()
    dy = torch.empty(n_out, dtype=torch.complex64, device="cuda")
    dho = torch.empty_like(dh)
    q(dx, dh, dho, dy, n_out, first)
    torch.cuda.synchronize()
    yq = dy.cpu().numpy()
    r = ref.ref64(x, h, D, p.phase_inc, first, hist)
    b = ref.bound(x, h, D, p.fft_size, r, hist)
    wp, wq = ref.worst(y, r, b), ref.worst(yq, r, b)
    d = float(np.max(np.abs(y.astype(np.complex128) - yq) / b))
    print(f"real {L} taps D={D}: {p.kernel} err/bound {wp:.4f}, {q.kernel} err/bound {wq:.4f}, difference/bound {d:.4f}")
    assert wp <= 1.0 and wq <= 1.0
    p.close()
    q.close()


@pytest.mark.parametrize("N,D,L,k0", [(1024, 8, 127, 0), (1024, 8, 127, 126), (2048, 64, 1000, 37), (8192, 4, 4096, 4095),
                                      (4096, 2, 33, 1)])
def test_impulse_tap(torch_cuda, N, D, L, k0):
    """h = c delta[k0]: y[m] = c x[mD - k0] times the phasor of that sample."""
    c = np.complex64(np.exp(0.7j))
    h = np.zeros(L, np.complex64)
    h[k0] = c
    first = 777
    p = nsh.FftXlatPlan(h, D, FREQ, fft_size=N)
    x = uniform(frames_len(p, p.tile + 1, 9), 3 * N + k0)
    y = run(torch_cuda, p, x, first=first)
    n_out = len(x) // D
    s = np.concatenate([np.zeros(L - 1), x.astype(np.complex128)])
    idx = np.arange(n_out) * D - k0
    r = np.complex128(c) * s[idx + L - 1] * np.exp(2j * np.pi * ref.turns(first, -k0, n_out * D - k0, p.phase_inc)[::D])
    w = ref.worst(y, r, ref.bound(x, h, D, N, r))
    print(f"impulse {p.kernel} L={L} k0={k0}: worst err/bound {w:.4f}")
    assert w <= 1.0
    p.close()


@pytest.mark.parametrize("N,D", [(1024, 8), (2048, 2), (4096, 64), (8192, 16)])
def test_tone_at_center_freq_comes_out_constant(torch_cuda, N, D):
    """A tone exactly at center_freq (its phase from the same 64-bit increment): every output past the
    filter's fill is sum(h), in magnitude and phase, across frame boundaries."""
    L = 200
    h = lowpass(L, D)
    first = (1 << 63) + 11
    p = nsh.FftXlatPlan(h, D, 0.3217, fft_size=N)
    n = frames_len(p, 2 * p.tile + 1, 1)
    x = tone(n, p.phase_inc, first).astype(np.complex64)
    y = run(torch_cuda, p, x, first=first)
    k = -(-L // D)
    dc = np.complex128(h.astype(np.complex128).sum())
    # the tone is rounded to fp32: 2^-24 of relative error a sample on top of the bound's terms
    tol = 1e-5 * abs(dc) + 1e-6 * np.abs(h).sum() + 2.0 ** -24 * np.abs(h).sum()
    e = np.abs(y[k:].astype(np.complex128) - dc)
    print(f"tone {p.kernel}: worst |y - sum h| / tolerance {np.max(e) / tol:.4f} over {len(y) - k} outputs")
    assert np.all(e <= tol)
    check("tone", p, x, h, y, None, first)
    p.close()


# ---- c. phase ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", [(1024, 8), (2048, 32), (4096, 2)])
@pytest.mark.parametrize("first_of", ["wraps", "2^40+3"])
def test_first_index(torch_cuda, N, D, first_of):
    first = (1 << 64) - 5 * D if first_of == "wraps" else (1 << 40) + 3  # 2^64 - 5 D: wraps inside the call
    h = lowpass(77, D)
    p = nsh.FftXlatPlan(h, D, FREQ, fft_size=N)
    x = signal(frames_len(p, p.tile, 11), p.phase_inc, 5)
    check("first " + first_of, p, x, h, run(torch_cuda, p, x, first=first), None, first, printed=True)
    p.close()


@pytest.mark.parametrize("N,D,L", [(1024, 8, 127), (2048, 4, 1024), (8192, 64, 300)])
def test_chained_calls(torch_cuda, N, D, L):
    """Two calls chained through hist_out -> hist_in with first_index advanced by n_out D, against one
    float64 reference of the whole stream; and the stream in one call. hist_out is bit-exact every
    time (run checks it)."""
    h = uniform(L, 3) * np.float32(0.05)
    p = nsh.FftXlatPlan(h, D, FREQ, fft_size=N)
    Vd = p.valid // D
    n1, n2 = (Vd + 33) * D, (2 * Vd + 5) * D
    first = (1 << 64) - n1 - 7  # the second call starts past the wrap
    x = signal(n1 + n2, p.phase_inc, 11 * N)
    hist0 = uniform(L - 1, 5)
    r = ref.ref64(x, h, D, p.phase_inc, first, hist0)
    s = np.concatenate([hist0, x])
    ya = run(torch_cuda, p, x[:n1], hist0, first)
    yb = run(torch_cuda, p, x[n1:], s[n1:n1 + L - 1], first + n1)
    for name, y, xi, hi, r_i in (("first call", ya, x[:n1], hist0, r[:n1 // D]),
                                 ("second call", yb, x[n1:], s[n1:n1 + L - 1], r[n1 // D:])):
        w = ref.worst(y, r_i, ref.bound(xi, h, D, N, r_i, hi))
        print(f"chained {p.kernel} {name}: worst err/bound {w:.4f}")
        assert w <= 1.0
    check("one call", p, x, h, run(torch_cuda, p, x, hist0, first), hist0, first)
    p.close()


@pytest.mark.parametrize("N,D", [(1024, 16), (4096, 4)])
def test_null_history_is_a_zero_history(torch_cuda, N, D):
    h = uniform(130, 4)
    p = nsh.FftXlatPlan(h, D, FREQ, fft_size=N)
    x = uniform(frames_len(p, p.tile, 3), 8)
    y0 = run(torch_cuda, p, x, None, 5)
    y1 = run(torch_cuda, p, x, np.zeros(129, np.complex64), 5)
    assert np.array_equal(bits(y0, np.complex64), bits(y1, np.complex64))
    p.close()


# ---- d. independence -------------------------------------------------------------------------------
@sizes
@pytest.mark.parametrize("D", [2, 16])
def test_grid_cap_does_not_change_the_bits(torch_cuda, N, D):
    h = uniform(127, 2)
    p = nsh.FftXlatPlan(h, D, FREQ, fft_size=N)
    x = uniform(frames_len(p, 4 * p.tile, 17), 31 + N)
    y0 = run(torch_cuda, p, x, first=3)
    for cap in (1, 3):
        p.grid_cap(cap)
        assert np.array_equal(bits(run(torch_cuda, p, x, first=3), np.complex64), bits(y0, np.complex64)), cap
    p.grid_cap(0)
    assert np.array_equal(bits(run(torch_cuda, p, x, first=3), np.complex64), bits(y0, np.complex64))
    check("grid cap", p, x, h, y0, None, 3)
    p.close()


@pytest.mark.parametrize("N,D,L", [(1024, 8, 127), (2048, 2, 1024), (4096, 32, 33), (8192, 4, 500)])
def test_appended_samples_leave_complete_frames_alone(torch_cuda, N, D, L):
    h = uniform(L, 12) * np.float32(0.1)
    p = nsh.FftXlatPlan(h, D, FREQ, fft_size=N)
    V, Vd = p.valid, p.valid // D
    x = uniform(6 * V + 40 * D, 41)
    n1 = (3 * Vd + 13) * D  # frames 0..2 end inside it: their windows end at 3V
    ya = run(torch_cuda, p, x[:n1], first=9)
    yb = run(torch_cuda, p, x, first=9)
    assert np.array_equal(bits(ya[:3 * Vd], np.complex64), bits(yb[:3 * Vd], np.complex64))
    check("short", p, x[:n1], h, ya, None, 9)
    check("long", p, x, h, yb, None, 9)
    p.close()


# ---- e. non-finite containment ---------------------------------------------------------------------
@pytest.mark.parametrize("N,D,L,where", [(1024, 8, 127, "overlap"), (1024, 64, 127, "middle"), (2048, 2, 1024, "overlap"),
                                         (4096, 16, 200, "overlap"), (8192, 4, 1, "middle")])
def test_nan_sample_stays_in_its_frames(torch_cuda, N, D, L, where):
    """One NaN sample among finite data: every output of every frame whose window holds it is
    non-finite, every other output has the clean run's bits."""
    h = uniform(L, 13)
    p = nsh.FftXlatPlan(h, D, FREQ, fft_size=N)
    V, O, Vd = p.valid, p.overlap, p.valid // D
    x = uniform(4 * V + 24 * D, 51)
    at = 2 * V - 1 if where == "overlap" and O else 2 * V + V // 2  # 2V-1: in frame 1's window and frame 2's
    clean = run(torch_cuda, p, x, first=1)
    xb = x.copy()
    xb[at] = complex(np.nan, 0.0)
    y = run(torch_cuda, p, xb, first=1)
    n_out = len(x) // D
    nf = -(-n_out // Vd)
    hit = [f for f in range(nf) if f * V - O <= at < f * V - O + N]
    assert len(hit) == (2 if where == "overlap" and O else 1)
    mask = np.zeros(n_out, bool)
    for f in hit:
        mask[f * Vd:(f + 1) * Vd] = True
    assert not np.any(np.isfinite(y[mask].real) & np.isfinite(y[mask].imag))
    assert np.array_equal(bits(y[~mask], np.complex64), bits(clean[~mask], np.complex64))
    p.close()


# ---- f. alignment ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,L", [(1024, 8, 127), (4096, 2, 2048), (8192, 64, 2)])
def test_eight_byte_alignment(torch_cuda, N, D, L):
    """in, out and both histories 8 bytes into their allocations (8-byte but not 16-byte aligned):
    the same bits as the aligned call, guards untouched (run checks two samples on each side)."""
    h = uniform(L, 14) * np.float32(0.05)
    p = nsh.FftXlatPlan(h, D, FREQ, fft_size=N)
    x = uniform(frames_len(p, p.tile + 1, 5), 21)
    hist = uniform(L - 1, 22)
    y0 = run(torch_cuda, p, x, hist, 3, odd=0)
    y1 = run(torch_cuda, p, x, hist, 3, odd=1)
    assert np.array_equal(bits(y0, np.complex64), bits(y1, np.complex64))
    check("aligned", p, x, h, y0, hist, 3)
    p.close()


# ---- g. what needs a device: the timing pair -------------------------------------------------------
def test_takes_the_armed_timing_pair(torch_cuda):
    torch = torch_cuda
    L = nsh.lib()

    def count():
        c = C.c_uint64()
        assert L.nsh_timed_launches(C.byref(c)) == 0
        return c.value

    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert L.nsh_event_create(C.byref(e)) == 0
    p = nsh.FftXlatPlan(uniform(127, 1), 8, FREQ)
    n = 1 << 16
    x = torch.zeros(n, dtype=torch.complex64, device="cuda")
    y = torch.empty(n // 8, dtype=torch.complex64, device="cuda")
    ho = torch.empty(126, dtype=torch.complex64, device="cuda")
    with pytest.raises(nsh.NshError, match="hist_out is required"):
        p(x, None, None, y, n // 8)
    c0 = count()
    assert L.nsh_time_next_launch(ev[0], ev[1]) == 0
    p(x, None, ho, y, n // 8)
    assert count() == c0 + 1
    p(x, None, ho, y, n // 8)  # unarmed: not counted
    assert count() == c0 + 1
    torch.cuda.synchronize()
    ms = C.c_float()
    assert L.nsh_event_elapsed_ms(ev[0], ev[1], C.byref(ms)) == 0 and ms.value > 0
    assert L.nsh_time_next_launch(ev[0], ev[1]) == 0
    p(x, None, ho, y, 0)  # nothing to do: the pair is dropped
    p(x, None, ho, y, n // 8)
    torch.cuda.synchronize()
    assert count() == c0 + 1
    for e in ev:
        L.nsh_event_destroy(e)
    p.close()
