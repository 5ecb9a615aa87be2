"""GPU: nsh_fft_c2c (the plan-based FFT, k_fft<N> and, for a plain 1024-point plan, k_fft1024) at all
ten sizes 16..8192, forward and inverse, with window and shift: the impulse basis, structured frames,
frame counts around the workgroup tile and the end of the buffer, the grid-stride walk under a grid
cap, frame independence, the bit identities of shift / window / the 1024-point kernel, non-finite
samples, power-of-two scaling, 8-byte-only aligned pointers, two streams, the armed timing pair and
the round trip.

Reference (float64, in this file): the complex64 input times the float32 window in double, then
numpy.fft.fft or N * numpy.fft.ifft on complex128, numpy.fft.fftshift on the output (forward) or the
input (inverse) of a shifted plan. Judged by oracle.tol_ok at the 1e-5 north-star bound per frame,
unless a test says bit-identical. Each tolerance test prints its worst frame's err / scale beside the
same ratio for scipy.fft on complex64 (a good fp32 transform; on the CPU it stays at or below 0.10 of
tol_ok's per-element bound at every size here); these ratios are reported here and asserted in
tests/test_gpu_fft_accuracy.py, which holds every size and direction to that transform's rms error."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from newsched_amd import nsh
from tests.gpu_util import bits, dev, hann, host, rand_window

pytestmark = pytest.mark.gpu

SIZES = [16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192]
DIRS = ["fwd", "inv"]
GUARD = complex(123.0, -77.0)
both = pytest.mark.parametrize("inv", [False, True], ids=DIRS)
sizes = pytest.mark.parametrize("N", SIZES)


def swap(a, N):
    """The halves of every frame of N swapped."""
    return np.ascontiguousarray(np.fft.fftshift(np.asarray(a).reshape(-1, N), axes=1)).ravel()


def ref(x, N, inv, w=None, shift=False):
    """The conventions in float64."""
    f = np.asarray(x, np.complex64).astype(np.complex128).reshape(-1, N)
    if w is not None:
        f = f * np.asarray(w, np.float32).astype(np.float64)[None, :]
    if not inv:
        y = np.fft.fft(f, axis=1)
        return (np.fft.fftshift(y, axes=1) if shift else y).ravel()
    if shift:
        f = np.fft.fftshift(f, axes=1)
    return (np.fft.ifft(f, axis=1) * N).ravel()


def yardstick(x, N, inv, w=None, shift=False):
    """A good fp32 transform of the same input: scipy.fft in complex64."""
    import scipy.fft as sf

    f = np.ascontiguousarray(x, np.complex64).reshape(-1, N)
    if w is not None:
        f = f * np.asarray(w, np.float32)[None, :]
    if not inv:
        y = sf.fft(f, axis=1)
        y = np.fft.fftshift(y, axes=1) if shift else y
    else:
        y = sf.ifft(np.fft.fftshift(f, axes=1) if shift else f, axis=1) * np.float32(N)
    assert y.dtype == np.complex64
    return y.ravel()


def run(torch, plan, x, in_off=0, out_off=0, tail=1024, stream=None):
    """plan over x with in / out each at a sample offset into a larger allocation; the output
    allocation holds out_off guard samples before the result and `tail` after it. Returns the result
    and checks every guard sample."""
    n = x.size
    N = plan.fft_size
    assert n % N == 0
    dx = torch.zeros(n + 2, dtype=torch.complex64, device="cuda")
    dx[in_off:in_off + n] = dev(torch, x)
    dy = torch.full((out_off + n + tail,), GUARD, dtype=torch.complex64, device="cuda")
    nsh.fft_c2c(plan, dx.data_ptr() + 8 * in_off, dy.data_ptr() + 8 * out_off, n // N, stream=stream)
    y = host(dy)
    g = np.complex64(GUARD)
    assert np.all(y[:out_off] == g) and np.all(y[out_off + n:] == g), (plan.kernel, n // N, in_off, out_off)
    return y[out_off:out_off + n]


def check_frames(name, y, r, N, yard=None):
    """tol_ok on every frame against its own scale (a frame whose reference is identically zero must
    be exactly zero); prints the worst frame's err / scale, and the yardstick's, and returns the
    frames that fail."""
    bad, worst, worst_y = [], 0.0, 0.0
    for f in range(y.size // N):
        s = slice(N * f, N * (f + 1))
        ok, err, scale = orc.tol_ok(y[s], r[s])
        if scale == 0:
            ok = bool(np.all(y[s] == 0))
        else:
            worst = max(worst, err / scale)
            if yard is not None:
                worst_y = max(worst_y, orc.tol_ok(yard[s], r[s])[1] / scale)
        if not ok:
            bad.append((f, err, scale))
    print("RATIO %s kernel %.3g scipy_fp32 %.3g" % (name, worst, worst_y))
    return bad


def tag(N, inv):
    return "N=%d %s" % (N, "inv" if inv else "fwd")


# ---- a. impulses -----------------------------------------------------------------------------
def impulse_positions(N):
    if N <= 1024:
        return np.arange(N)
    fixed = [0, 1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, N // 2 - 1, N // 2, N // 2 + 1, N - 1]
    return np.array(fixed + list(np.random.default_rng(N).integers(0, N, 32)))


@sizes
@both
def test_impulses(torch_cuda, N, inv):
    """Frame i a unit impulse at p_i (the whole basis up to 1024 points): row p_i of the DFT matrix
    (its conjugate for the inverse). Every entry has modulus 1 and must be met within 1.1e-5, while
    a wrong twiddle index, digit reversal or pad slip moves one by at least 2 sin(pi / N) >= 7.7e-4."""
    pos = impulse_positions(N)
    x = np.zeros((pos.size, N), np.complex64)
    x[np.arange(pos.size), pos] = 1
    y = run(torch_cuda, nsh.FftPlan(N, inv), x.ravel())
    pk = (pos[:, None] * np.arange(N)[None, :]) % N
    dft = np.exp((2j if inv else -2j) * np.pi * pk / N).ravel()
    err = np.abs(y - dft).max()
    print("RATIO a/impulses %s kernel %.3g (absolute, bound 1.1e-5)" % (tag(N, inv), err))
    assert err <= 1.1e-5


# ---- b. structured frames --------------------------------------------------------------------
def structured_frames(N):
    n = np.arange(N)
    rng = np.random.default_rng(7)
    fr = [("dc", np.full(N, 0.5 + 0.25j)), ("nyquist", (-1.0) ** n + 0j)]
    for k in (1, N // 16 - 1, N // 16, N // 16 + 1, N // 2, N - 1):
        fr.append(("tone%d" % k, np.exp(2j * np.pi * k * n / N)))  # in double, rounded to complex64 below
    fr += [("real", rng.uniform(-1, 1, N) + 0j), ("imag", 1j * rng.uniform(-1, 1, N)), ("zero", np.zeros(N, complex))]
    return [k for k, _ in fr], np.concatenate([v.astype(np.complex64) for _, v in fr])


@sizes
@both
def test_structured_frames(torch_cuda, N, inv):
    """DC, Nyquist, single tones, purely real / imaginary and all-zero frames in one batch, each
    within tolerance on its own frame's scale. The DC frame's sums are sums of equal values scaled by
    powers of two, hence exact: bin 0 equals N c. The zero frame's output is exactly zero."""
    names, x = structured_frames(N)
    y = run(torch_cuda, nsh.FftPlan(N, inv), x)
    bad = check_frames("b/structured %s" % tag(N, inv), y, ref(x, N, inv), N, yardstick(x, N, inv))
    assert not bad, [(names[f], e, s) for f, e, s in bad]
    assert y[0] == np.complex64(N * (0.5 + 0.25j))
    z = names.index("zero")
    assert np.all(y[N * z:N * (z + 1)] == 0)


# ---- c. frame counts, the end of the buffer, the grid cap ------------------------------------
_big = {}


def big_batch(N, inv):
    """5 T + 1 frames (at least 37) and their reference, computed once per (N, direction)."""
    if (N, inv) not in _big:
        p = nsh.FftPlan(N, inv)
        nf = max(5 * p.tile + 1, 37)
        x = orc.synth(nf * N, 100 + N)
        r = ref(x, N, inv)
        for a in (x, r):
            a.setflags(write=False)
        _big[(N, inv)] = (p.tile, x, r)
    return _big[(N, inv)]


@sizes
@both
def test_frame_counts_and_buffer_end(torch_cuda, N, inv):
    """Counts around the workgroup's tile T (partly filled waves, teams and workgroups, and the
    prefetch of the tile one stride past the end): results within tolerance, 2 guard samples before
    the output and 1024 after it unchanged."""
    T, x, r = big_batch(N, inv)
    p = nsh.FftPlan(N, inv)
    for nf in sorted({1, T - 1, T, T + 1, 2 * T + 1, 37} - {0}):
        y = run(torch_cuda, p, x[:nf * N], out_off=2)
        bad = check_frames("c/nframes=%d %s" % (nf, tag(N, inv)), y, r[:nf * N], N)
        assert not bad, (nf, bad[:4])


@sizes
@both
def test_grid_cap_walks_the_stride(torch_cuda, N, inv):
    """With at most 2 workgroups, 5 T + 1 frames take the grid-stride walk through three steps (the
    second workgroup's last one past the end): bit-identical to the uncapped run, and within tolerance."""
    T, x, r = big_batch(N, inv)
    p = nsh.FftPlan(N, inv)
    y0 = run(torch_cuda, p, x)
    assert not check_frames("c/batch %s" % tag(N, inv), y0, r, N, yardstick(x, N, inv))
    p.grid_cap(2)
    y2 = run(torch_cuda, p, x)
    np.testing.assert_array_equal(bits(y2), bits(y0))
    p.grid_cap(0)
    np.testing.assert_array_equal(bits(run(torch_cuda, p, x)), bits(y0))


# ---- d. frame independence -------------------------------------------------------------------
@sizes
@both
def test_frame_independent_of_batch_and_slot(torch_cuda, N, inv):
    """A frame's output does not depend on its neighbours, its slot in the wave or workgroup or the
    batch size: frames 0, 1, T - 1, T and the last one alone, and five from the middle as a batch,
    bit-identical to the batch of 5 T + 1 (at N = 16 a wave holds 64 frames)."""
    T, x, _ = big_batch(N, inv)
    p = nsh.FftPlan(N, inv)
    big = run(torch_cuda, p, x)
    nf = x.size // N
    for f in sorted({0, 1, T - 1, T, nf - 1}):
        one = run(torch_cuda, p, x[N * f:N * (f + 1)])
        np.testing.assert_array_equal(bits(one), bits(big[N * f:N * (f + 1)]), err_msg="frame %d" % f)
    m = nf // 2
    five = run(torch_cuda, p, x[N * m:N * (m + 5)])
    np.testing.assert_array_equal(bits(five), bits(big[N * m:N * (m + 5)]))


# ---- e. bit identities -----------------------------------------------------------------------
@sizes
def test_forward_shift_is_the_swapped_output(torch_cuda, N):
    x = orc.synth(7 * N, 40)
    w = rand_window(N)
    for win in (None, w):
        plain = run(torch_cuda, nsh.FftPlan(N, False, win), x)
        shifted = run(torch_cuda, nsh.FftPlan(N, False, win, shift=True), x)
        np.testing.assert_array_equal(bits(shifted), bits(swap(plain, N)))


@sizes
def test_inverse_shift_is_the_swapped_input(torch_cuda, N):
    """Inverse with shift of (x, w) == inverse without shift of (swap(x), swap(w)): the window is
    indexed by the input position as it arrives."""
    x = orc.synth(7 * N, 41)
    w = rand_window(N)
    a = run(torch_cuda, nsh.FftPlan(N, True, w, shift=True), x)
    b = run(torch_cuda, nsh.FftPlan(N, True, swap(w, N)), swap(x, N))
    np.testing.assert_array_equal(bits(a), bits(b))
    a = run(torch_cuda, nsh.FftPlan(N, True, None, shift=True), x)
    b = run(torch_cuda, nsh.FftPlan(N, True), swap(x, N))
    np.testing.assert_array_equal(bits(a), bits(b))


@sizes
@both
def test_ones_window_is_no_window(torch_cuda, N, inv):
    x = orc.synth(7 * N, 42)
    a = run(torch_cuda, nsh.FftPlan(N, inv, np.ones(N, np.float32)), x)
    b = run(torch_cuda, nsh.FftPlan(N, inv), x)
    np.testing.assert_array_equal(bits(a), bits(b))


@both
def test_plain_1024_is_fft1024(torch_cuda, inv):
    torch = torch_cuda
    x = orc.synth(37 * 1024, 100)
    p = nsh.FftPlan(1024, inv)
    assert p.kernel.startswith("k_fft1024")
    y = run(torch, p, x)
    dx = dev(torch, x)
    dy = torch.empty_like(dx)
    nsh.fft1024(dx, dy, 37, inverse=inv)
    np.testing.assert_array_equal(bits(y), bits(host(dy)))
    # ... and so is the generic kernel that a window or a shift selects at 1024
    q = nsh.FftPlan(1024, inv, np.ones(1024, np.float32))
    assert q.kernel.startswith("k_fft<1024")
    np.testing.assert_array_equal(bits(run(torch, q, x)), bits(y))


# ---- f. windows ------------------------------------------------------------------------------
@sizes
@both
@pytest.mark.parametrize("shift", [False, True], ids=["plain", "shift"])
def test_windows_against_reference(torch_cuda, N, inv, shift):
    """Hann and a random window on random frames, an impulse frame at every eighth position and on the
    Hann window's zero first sample (reference identically zero: the output must be exactly zero)."""
    x = orc.synth(9 * N, 43 + N).reshape(9, N).copy()
    x[7] = 0
    x[7, ::8] = 1
    x[8] = 0
    x[8, 0] = 1 - 1j
    x = x.ravel()
    for wname, w in (("hann", hann(N)), ("random", rand_window(N))):
        y = run(torch_cuda, nsh.FftPlan(N, inv, w, shift), x)
        r = ref(x, N, inv, w, shift)
        bad = check_frames("f/%s%s %s" % (wname, "+shift" if shift else "", tag(N, inv)), y, r, N,
                           yardstick(x, N, inv, w, shift))
        assert not bad, (wname, bad)
        if wname == "hann":
            assert np.all(r[8 * N:] == 0) and np.all(y[8 * N:] == 0)


@sizes
@both
def test_power_of_two_window_scales_exactly(torch_cuda, N, inv):
    x = orc.synth(5 * N, 44)
    a = run(torch_cuda, nsh.FftPlan(N, inv, np.full(N, 0.125, np.float32)), x)
    b = run(torch_cuda, nsh.FftPlan(N, inv), x)
    np.testing.assert_array_equal(bits(a), bits(b * np.float32(0.125)))


# ---- g. non-finite containment ---------------------------------------------------------------
_NAN, _INF = float("nan"), float("inf")


@sizes
@both
@pytest.mark.parametrize("bad", [complex(_NAN, _NAN), complex(_INF, 0.0), complex(0.25, -_INF)],
                         ids=["nan+nanj", "inf+0j", "0.25-infj"])
def test_nonfinite_sample_stays_in_its_frame(torch_cuda, N, inv, bad):
    """One bad sample at index min(77, N - 3) of frame 1 of 3: frames 0 and 2 are bit-identical to the
    clean run, every output of frame 1 is non-finite. At N = 16 and 64 (several frames per lane group
    of a wave) also with the bad frame in the middle of a wave's 1024 / N frames."""
    p = nsh.FftPlan(N, inv)
    cases = [(3, 1)] + ([(1024 // N, 512 // N)] if N in (16, 64) else [])
    for nf, fb in cases:
        x = orc.synth(nf * N, 21)
        clean = run(torch_cuda, p, x)
        xb = x.copy()
        xb[fb * N + min(77, N - 3)] = bad
        y = run(torch_cuda, p, xb)
        keep = np.ones(nf * N, bool)
        keep[fb * N:(fb + 1) * N] = False
        np.testing.assert_array_equal(bits(y[keep]), bits(clean[keep]))
        mid = y[fb * N:(fb + 1) * N]
        nonfinite = ~np.isfinite(mid.real) | ~np.isfinite(mid.imag)
        assert nonfinite.all(), (N, inv, bad, nf, int((~nonfinite).sum()), np.nonzero(~nonfinite)[0][:8].tolist())


# ---- h. power-of-two homogeneity -------------------------------------------------------------
@sizes
@both
def test_power_of_two_scaling_is_exact(torch_cuda, N, inv):
    """fft(s x) == s fft(x) bit for bit for s = 2^-60, 2^60, 2^90: synthetic samples are multiples of
    2^-23 in [-1, 1) and the growth is at most 8192 sqrt(2), so nothing under- or overflows."""
    x = orc.synth(5 * N, 22)
    p = nsh.FftPlan(N, inv)
    y = run(torch_cuda, p, x)
    for e in (-60, 60, 90):
        s = np.float32(2.0 ** e)
        np.testing.assert_array_equal(bits(run(torch_cuda, p, x * s)), bits(y * s), err_msg="2^%d" % e)


# ---- i. odd sample offsets -------------------------------------------------------------------
@sizes
@both
def test_odd_sample_offsets(torch_cuda, N, inv):
    """in and out each one complex sample (8 bytes) into a larger allocation: bit-identical to the
    16-byte aligned run, the guards before and after the output intact (checked in run())."""
    x = orc.synth(5 * N, 24)
    p = nsh.FftPlan(N, inv, hann(N), shift=True)
    y0 = run(torch_cuda, p, x, out_off=2)
    for in_off, out_off in [(1, 2), (0, 1), (1, 1), (1, 3)]:
        y = run(torch_cuda, p, x, in_off=in_off, out_off=out_off)
        np.testing.assert_array_equal(bits(y), bits(y0), err_msg=str((in_off, out_off)))


# ---- j. two streams --------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 512, 8192])
def test_two_streams_back_to_back(torch_cuda, N):
    """Two plans (forward windowed, inverse shifted) on two streams, issued back to back: each
    bit-identical to the same call on the current stream."""
    torch = torch_cuda
    nf = 37
    plans = [nsh.FftPlan(N, False, hann(N)), nsh.FftPlan(N, True, None, shift=True)]
    xs = [dev(torch, orc.synth(nf * N, 100)), dev(torch, orc.synth(nf * N, 31))]
    want = [torch.empty_like(x) for x in xs]
    for p, x, y in zip(plans, xs, want):
        nsh.fft_c2c(p, x, y, nf)
    got = [torch.full_like(x, GUARD) for x in xs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for p, x, y, s in zip(plans, xs, got, streams):
        nsh.fft_c2c(p, x, y, nf, stream=s)
    for s in streams:
        s.synchronize()
    for y, r in zip(got, want):
        np.testing.assert_array_equal(bits(host(y)), bits(host(r)))


# ---- k. the armed timing pair ----------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 1024, 4096])
def test_fft_takes_the_armed_timing_pair(torch_cuda, N):
    """An armed nsh_time_next_launch pair is taken by exactly one launch of nsh_fft_c2c
    (nsh_timed_launches + 1, positive elapsed time); a call with nframes = 0 launches nothing and
    drops the pair, so the next, unarmed launch is not timed. 1024: the plain plan (k_fft1024)."""
    torch = torch_cuda
    L = nsh.lib()

    def count():
        c = C.c_uint64()
        assert L.nsh_timed_launches(C.byref(c)) == 0
        return c.value

    def events():
        ev = [C.c_void_p(), C.c_void_p()]
        for e in ev:
            assert L.nsh_event_create(C.byref(e)) == 0
        return ev

    nf = (1 << 18) // N
    x = dev(torch, orc.synth(nf * N, 11))
    y = torch.empty_like(x)
    p = nsh.FftPlan(N)
    ev = events()
    c0 = count()
    assert L.nsh_time_next_launch(ev[0], ev[1]) == 0
    nsh.fft_c2c(p, x, y, nf)
    assert count() == c0 + 1
    nsh.fft_c2c(p, x, y, nf)  # unarmed: not counted
    assert count() == c0 + 1
    torch.cuda.synchronize()
    ms = C.c_float()
    assert L.nsh_event_elapsed_ms(ev[0], ev[1], C.byref(ms)) == 0 and ms.value > 0
    for e in ev:
        L.nsh_event_destroy(e)
    ev = events()
    c0 = count()
    assert L.nsh_time_next_launch(ev[0], ev[1]) == 0
    nsh.fft_c2c(p, x, y, 0)   # nothing to do: no launch, the pair is dropped on return
    nsh.fft_c2c(p, x, y, nf)  # unarmed
    torch.cuda.synchronize()
    assert count() == c0
    assert L.nsh_event_elapsed_ms(ev[0], ev[1], C.byref(ms)) != 0  # never recorded
    for e in ev:
        L.nsh_event_destroy(e)


# ---- l. round trip ---------------------------------------------------------------------------
@sizes
def test_round_trip(torch_cuda, N):
    """inverse(forward(x)) / N against x (the division by a power of two is exact)."""
    torch = torch_cuda
    nf = 11
    x = orc.synth(nf * N, 50 + N)
    mid = run(torch, nsh.FftPlan(N, False), x)
    back = run(torch, nsh.FftPlan(N, True), mid) / np.float32(N)
    bad = check_frames("l/round trip N=%d" % N, back, x.astype(np.complex128), N)
    assert not bad, bad
