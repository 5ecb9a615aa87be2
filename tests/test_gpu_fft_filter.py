"""GPU: nsh_fft_filter_ccc (k_fft_xlat<N, 1, false>, overlap-save FIR with complex taps) at its four frame
sizes through the fft_size override and under the default size rule on each side of its boundaries.

Reference (float64, ref64 here): numpy.convolve of hist_in ++ in with the taps, both complex128.
The header's bound (tests/fft_xlat_ref.py's at D = 1), per output m of frame f = m // V of a call:
    |y - y_ref| <= 1e-5 |y_ref| + 1e-6 * max|x over frame f's window| * sum_k |h[k]|
Every tolerance test prints its worst err / bound beside the same ratio of an overlap-save with
scipy.fft in complex64 on the same frames (a good fp32 transform); that ratio is reported here and
asserted in tests/test_gpu_fft_accuracy.py, which holds the kernel at every N to the rms error of the
complex64 chain. hist_out is bit-exact in every test that runs the kernel.

Measured on one MI355X (worst err / bound over this file): see DESIGN.md section 4.8."""
import ctypes as C

import numpy as np
import pytest

from newsched_amd import nsh
from tests import fft_xlat_ref as ref
from tests.fft_xlat_ref import SIZES, rule, worst
from tests.gpu_util import bits, uniform

pytestmark = pytest.mark.gpu

GUARD = complex(123.0, -77.0)
NG = 2  # guard samples on each side of out and hist_out
sizes = pytest.mark.parametrize("N", SIZES)


def taps_of(kind, L):
    import scipy.signal as ss

    if kind == "firwin":
        return ss.firwin(L, 0.25).astype(np.complex64)
    if kind == "random":
        return uniform(L, 1000 + L)
    # one-sided (analytic) band-pass: the low-pass moved to +0.2 cycles per sample
    return (ss.firwin(L, 0.15) * np.exp(2j * np.pi * 0.2 * np.arange(L))).astype(np.complex64)


def ref64(x, h, hist=None):
    H = len(h) - 1
    return np.convolve(ref.stream_of(x, hist, H), np.asarray(h, np.complex64).astype(np.complex128))[H:H + len(x)]


def standin(x, h, N, hist=None):
    """Overlap-save over the same frames with scipy.fft in complex64."""
    import scipy.fft as sf

    H, n = len(h) - 1, len(x)
    V = N - H
    nf = -(-n // V)
    s = np.concatenate([ref.stream_of(x, hist, H), np.zeros(nf * V + N)]).astype(np.complex64)
    Hs = np.fft.fft(np.asarray(h, np.complex128), N).astype(np.complex64)
    w = np.stack([s[f * V:f * V + N] for f in range(nf)])
    y = sf.ifft(sf.fft(w, axis=1) * Hs[None, :], axis=1)
    assert y.dtype == np.complex64
    return y[:, H:].ravel()[:n]


def run(torch, plan, x, hist=None, odd=0, want_hist=True):
    """One call over x with every pointer `odd` samples (8 bytes each) into its allocation, NG guard
    samples on each side of out and hist_out; checks the guards and hist_out's bits; returns out."""
    n, H = len(x), plan.hist_len
    dx = torch.zeros(odd + n, dtype=torch.complex64, device="cuda")
    dx[odd:] = torch.from_numpy(np.array(x, np.complex64)).cuda()
    dy = torch.full((odd + NG + n + NG,), GUARD, dtype=torch.complex64, device="cuda")
    dho = torch.full((odd + NG + H + NG,), GUARD, dtype=torch.complex64, device="cuda")
    dhi = None
    if hist is not None:
        dhi = torch.zeros(odd + H, dtype=torch.complex64, device="cuda")
        dhi[odd:] = torch.from_numpy(np.array(hist, np.complex64)).cuda()
    plan(dx.data_ptr() + 8 * odd, None if dhi is None else dhi.data_ptr() + 8 * odd,
         dho.data_ptr() + 8 * (odd + NG) if (H or want_hist) else None, dy.data_ptr() + 8 * (odd + NG), n)
    torch.cuda.synchronize()
    y, ho = dy.cpu().numpy(), dho.cpu().numpy()
    g = np.complex64(GUARD)
    assert np.all(y[:odd + NG] == g) and np.all(y[odd + NG + n:] == g), (plan.kernel, n, odd)
    assert np.all(ho[:odd + NG] == g) and np.all(ho[odd + NG + H:] == g), (plan.kernel, n, odd)
    tail = np.concatenate([np.zeros(H, np.complex64) if hist is None else np.asarray(hist, np.complex64),
                           np.asarray(x, np.complex64)])[n:]
    assert np.array_equal(bits(ho[odd + NG:odd + NG + H], np.complex64), bits(tail, np.complex64)), (plan.kernel, n, "hist_out")
    return y[odd + NG:odd + NG + n]


def check(name, plan, x, h, y, hist=None, printed=True):
    N = plan.fft_size
    r = ref64(x, h, hist)
    b = ref.bound(x, h, 1, N, r, hist)
    w = worst(y, r, b)
    if printed:
        print(f"{name} {plan.kernel} L={len(h)} n={len(x)}: worst err/bound {w:.4f}, "
              f"scipy complex64 overlap-save {worst(standin(x, h, N, hist), r, b):.4f}")
    assert w <= 1.0, (name, plan.kernel, len(h), w)
    return w


def sweep_len(plan):
    return 2 * plan.tile * plan.valid + 17  # more than one workgroup step and a partial last frame


# ---- a. parity at every size ---------------------------------------------------------------------
@sizes
@pytest.mark.parametrize("Lk", ["1", "2", "127", "N/2-1", "N/2"])
@pytest.mark.parametrize("kind", ["firwin", "random", "analytic"])
def test_parity(torch_cuda, N, Lk, kind):
    L = {"1": 1, "2": 2, "127": 127, "N/2-1": N // 2 - 1, "N/2": N // 2}[Lk]
    h = taps_of(kind, L)
    p = nsh.FftFilterPlan(h, N)
    assert (p.fft_size, p.valid, p.hist_len, p.kernel) == (N, N - (L - 1), L - 1, f"k_fft_xlat<{N}, 1, false>")
    x = uniform(sweep_len(p), N + L)
    check("parity " + kind, p, x, h, run(torch_cuda, p, x))
    p.close()


# ---- b. the default size rule, each side of each boundary ------------------------------------------
@pytest.mark.parametrize("L", [1, 256, 257, 512, 513, 2048, 2049, 4096])
def test_default_size_rule(torch_cuda, L):
    h = taps_of("random", L)
    p = nsh.FftFilterPlan(h)
    N = rule(L)
    lib = nsh.lib()
    assert lib.nsh_fft_filter_fft_size(p._h) == N
    assert lib.nsh_fft_filter_valid(p._h) == N - (L - 1)
    assert lib.nsh_fft_filter_history(p._h) == L - 1
    assert lib.nsh_fft_filter_kernel(p._h) == b"k_fft_xlat<%d, 1, false>" % N
    assert lib.nsh_fft_filter_tile(p._h) == max(1, 4096 // N)
    x = uniform(sweep_len(p), 7 + L)
    check("default rule", p, x, h, run(torch_cuda, p, x))
    p.close()


# ---- c. impulse taps: window start, valid range and spectrum order ---------------------------------
@sizes
@pytest.mark.parametrize("Lk", ["127", "N/2"])
@pytest.mark.parametrize("k0k", ["0", "1", "L-1"])
def test_impulse_taps(torch_cuda, N, Lk, k0k):
    L = 127 if Lk == "127" else N // 2
    k0 = {"0": 0, "1": 1, "L-1": L - 1}[k0k]
    c = np.complex64(np.exp(0.7j))
    h = np.zeros(L, np.complex64)
    h[k0] = c
    p = nsh.FftFilterPlan(h, N)
    x = uniform(sweep_len(p), 3 * N + k0)
    y = run(torch_cuda, p, x)
    # the delayed input times c, in double
    r = np.concatenate([np.zeros(k0), x.astype(np.complex128)])[:len(x)] * np.complex128(c)
    b = ref.bound(x, h, 1, N, r)
    w = worst(y, r, b)
    print(f"impulse {p.kernel} L={L} k0={k0}: worst err/bound {w:.4f}")
    assert w <= 1.0
    p.close()


# ---- d. chained calls --------------------------------------------------------------------------
@pytest.mark.parametrize("N,L", [(1024, 127), (2048, 1024), (8192, 300)])
def test_chained_calls(torch_cuda, N, L):
    """Calls cut at an odd sample, a call of one sample, a call shorter than the history (its hist_out
    mixes hist_in and in) and the rest, chained through hist_out -> hist_in from a non-zero initial
    history; and the same stream in one call. Every call is within the bound of float64 for its own
    frames; hist_out is bit-exact every time (run checks it)."""
    h = taps_of("random", L)
    p = nsh.FftFilterPlan(h, N)
    V = p.valid
    short = min(50, L - 2)
    cuts = [(V + 333) | 1, 1, short, 2 * V + 5]  # the first cut odd and no multiple of V
    x = uniform(sum(cuts), 11 * N)
    hist0 = uniform(L - 1, 5)
    s = np.concatenate([hist0, x])
    at = 0
    for i, n in enumerate(cuts):
        hist = s[at:at + L - 1]
        xi = x[at:at + n]
        y = run(torch_cuda, p, xi, hist)
        check(f"chained call {i}", p, xi, h, y, hist)
        at += n
    check("one call", p, x, h, run(torch_cuda, p, x, hist0), hist0)
    p.close()


# ---- e. alignment and guards -----------------------------------------------------------------------
@pytest.mark.parametrize("N,L", [(1024, 127), (4096, 2048), (8192, 2)])
def test_eight_byte_alignment(torch_cuda, N, L):
    """in, out and both histories 8 bytes into their allocations (8-byte but not 16-byte aligned):
    the same bits as the aligned call, guards untouched (run checks two samples on each side)."""
    h = taps_of("analytic", L)
    p = nsh.FftFilterPlan(h, N)
    x = uniform(sweep_len(p), 21)
    hist = uniform(L - 1, 22)
    y0 = run(torch_cuda, p, x, hist, odd=0)
    y1 = run(torch_cuda, p, x, hist, odd=1)
    assert np.array_equal(bits(y0, np.complex64), bits(y1, np.complex64))
    check("aligned", p, x, h, y0, hist)
    p.close()


# ---- f. grid cap -------------------------------------------------------------------------------
@sizes
def test_grid_cap_does_not_change_the_bits(torch_cuda, N):
    h = taps_of("random", 127)
    p = nsh.FftFilterPlan(h, N)
    x = uniform(5 * p.tile * p.valid + 17, 31 + N)
    y0 = run(torch_cuda, p, x)
    for cap in (1, 2):
        p.grid_cap(cap)
        assert np.array_equal(bits(run(torch_cuda, p, x), np.complex64), bits(y0, np.complex64)), cap
    p.grid_cap(0)
    assert np.array_equal(bits(run(torch_cuda, p, x), np.complex64), bits(y0, np.complex64))
    check("grid cap", p, x, h, y0)
    p.close()


@pytest.mark.parametrize("N", [1024, 8192])  # Hs in registers, Hs re-read every frame
def test_one_history_sample_at_the_frame_zero_seam(torch_cuda, N):
    """L = 2: H = 1, so frame 0's window is exactly one history sample (non-zero here) and then the
    input. One workgroup walks 2 tile + 1 frames: frame 0, a prefetched second trip and a partial
    last frame. An overlap or a first index other than L - 1 and 0 shows at out[0] and at every frame
    start; run checks hist_out's bits."""
    h = taps_of("random", 2)
    p = nsh.FftFilterPlan(h, N)
    assert (p.valid, p.hist_len) == (N - 1, 1)
    p.grid_cap(1)
    x = uniform(2 * p.tile * p.valid + 17, 35 + N)
    hist = np.array([3.0 - 2.0j], np.complex64)
    check("frame-0 seam", p, x, h, run(torch_cuda, p, x, hist), hist)
    p.close()


# ---- g. frame independence ---------------------------------------------------------------------
@pytest.mark.parametrize("N,L", [(1024, 127), (2048, 1024), (4096, 33)])
def test_appended_samples_leave_complete_frames_alone(torch_cuda, N, L):
    h = taps_of("firwin", L)
    p = nsh.FftFilterPlan(h, N)
    V = p.valid
    x = uniform(7 * V + 300, 41)
    n1 = 3 * V + 123  # frames 0..2 end inside it: their windows end at 3V
    ya = run(torch_cuda, p, x[:n1])
    yb = run(torch_cuda, p, x)
    assert np.array_equal(bits(ya[:3 * V], np.complex64), bits(yb[:3 * V], np.complex64))
    check("short", p, x[:n1], h, ya, printed=False)
    check("long", p, x, h, yb, printed=False)
    p.close()


# ---- h. non-finite containment -----------------------------------------------------------------
@pytest.mark.parametrize("bad", [complex(np.nan, 0.0), complex(0.25, np.inf)], ids=["nan", "inf"])
@pytest.mark.parametrize("N,L,where", [(1024, 127, "overlap"), (1024, 127, "middle"), (2048, 1024, "overlap"),
                                       (8192, 1, "middle")])
def test_nonfinite_sample_stays_in_its_frames(torch_cuda, bad, N, L, where):
    """One non-finite sample among finite data: every output of every frame whose window holds it is
    non-finite, every other output has the clean run's bits."""
    h = taps_of("random", L)
    p = nsh.FftFilterPlan(h, N)
    V, H = p.valid, L - 1
    x = uniform(4 * V + 99, 51)
    at = 2 * V - 1 if where == "overlap" and H else 2 * V + V // 2  # 2V-1: in frame 1's window and frame 2's
    clean = run(torch_cuda, p, x)
    xb = x.copy()
    xb[at] = bad
    y = run(torch_cuda, p, xb)
    nf = -(-len(x) // V)
    hit = [f for f in range(nf) if f * V - H <= at < (f + 1) * V]
    assert len(hit) == (2 if where == "overlap" and H else 1)
    mask = np.zeros(len(x), bool)
    for f in hit:
        mask[f * V:(f + 1) * V] = True
    assert not np.any(np.isfinite(y[mask].real) & np.isfinite(y[mask].imag))
    assert np.array_equal(bits(y[~mask], np.complex64), bits(clean[~mask], np.complex64))
    p.close()


# ---- i. against the direct form ------------------------------------------------------------------
def test_against_the_direct_form(torch_cuda):
    """127 real taps: nsh_fft_filter_ccc and nsh_fir_ccf(NSH_FIR_DIRECT) on the same data, each judged
    against float64 under this file's bound; both ratios printed. No bit identity is expected."""
    import scipy.signal as ss

    torch = torch_cuda
    hr = ss.firwin(127, 0.25).astype(np.float32)
    h = hr.astype(np.complex64)
    p = nsh.FftFilterPlan(h)
    x = uniform(sweep_len(p), 61)
    y = run(torch, p, x)
    d = nsh.FirPlan(hr, 1, nsh.FIR_DIRECT)
    dx = torch.from_numpy(x).cuda()
    hin = torch.zeros(126, dtype=torch.complex64, device="cuda")
    hout = torch.zeros_like(hin)
    dy = torch.empty_like(dx)
    d(dx, hin, hout, dy, len(x))
    torch.cuda.synchronize()
    r = ref64(x, h)
    b = ref.bound(x, h, 1, p.fft_size, r)
    wf, wd = worst(y, r, b), worst(dy.cpu().numpy(), r, b)
    print(f"real 127 taps: {p.kernel} err/bound {wf:.4f}, {d.kernel} err/bound {wd:.4f}")
    assert wf <= 1.0 and wd <= 1.0
    d.close()
    p.close()


# ---- j. what needs a plan: the missing hist_out, the timing pair --------------------------------
def test_missing_hist_out_is_refused_unless_there_is_no_history(torch_cuda):
    torch = torch_cuda
    x = torch.zeros(64, dtype=torch.complex64, device="cuda")
    y = torch.empty_like(x)
    p = nsh.FftFilterPlan(np.ones(2, np.complex64))
    with pytest.raises(nsh.NshError, match="hist_out is required"):
        p(x, None, None, y, 64)
    p.close()
    p = nsh.FftFilterPlan(np.array([2j], np.complex64))
    xs = uniform(3000, 71)
    yy = run(torch, p, xs, want_hist=False)  # one tap: no history, hist_out may be NULL
    check("one tap", p, xs, np.array([2j], np.complex64), yy, printed=False)
    p.close()


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
    p = nsh.FftFilterPlan(taps_of("random", 127))
    n = 1 << 16
    x = torch.zeros(n, dtype=torch.complex64, device="cuda")
    y = torch.empty_like(x)
    ho = torch.empty(126, dtype=torch.complex64, device="cuda")
    c0 = count()
    assert L.nsh_time_next_launch(ev[0], ev[1]) == 0
    p(x, None, ho, y, n)
    assert count() == c0 + 1
    p(x, None, ho, y, n)  # unarmed: not counted
    assert count() == c0 + 1
    torch.cuda.synchronize()
    ms = C.c_float()
    assert L.nsh_event_elapsed_ms(ev[0], ev[1], C.byref(ms)) == 0 and ms.value > 0
    assert L.nsh_time_next_launch(ev[0], ev[1]) == 0
    p(x, None, ho, y, 0)  # nothing to do: the pair is dropped
    p(x, None, ho, y, n)
    torch.cuda.synchronize()
    assert count() == c0 + 1
    for e in ev:
        L.nsh_event_destroy(e)
    p.close()
