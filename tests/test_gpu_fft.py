"""GPU: nsh_fft1024_c2c (k_fft1024) and nsh_channelizer1024 (k_chan1024) at the edges their three
tests in test_gpu_kernels.py leave out: frame counts that are no multiple of the four frames a
workgroup runs, the end of the buffer, frame independence, the whole operator on the impulse basis,
structured and far-from-O(1) inputs, non-finite samples, 8-byte-only aligned pointers, the
channelizer against its staged form, two streams and the armed timing pair.

Reference: oracle.fft1024 / oracle.channelizer1024 (double precision), judged by oracle.tol_ok at
the 1e-5 north-star bound, unless a test says bit-identical. Each tolerance test prints its measured
err / scale beside the same ratio for scipy.fft on the complex64 input (a good fp32 transform);
these ratios are reported here and asserted in tests/test_gpu_fft_accuracy.py (rms error against that
transform's)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from newsched_amd import nsh
from tests.gpu_util import bits, dev, host

pytestmark = pytest.mark.gpu

OPS = ["fwd", "inv", "chan"]
GUARD = complex(123.0, -77.0)


def rand_w(seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, 1024) + 1j * rng.uniform(-1, 1, 1024)).astype(np.complex64)


W = rand_w(1)  # the random complex weights of every channelizer case that names no other
_refs = {}


def ref(op, x, w=W, key=None):
    """The oracle's result; with a key, computed once and shared (returned read-only)."""
    if key is not None and (op, key) in _refs:
        return _refs[(op, key)]
    r = orc.channelizer1024(x, w) if op == "chan" else orc.fft1024(x, inverse=(op == "inv"))
    if key is not None:
        r.setflags(write=False)
        _refs[(op, key)] = r
    return r


def yardstick(op, x, w=W):
    """A good fp32 transform of the same input: scipy.fft in complex64."""
    import scipy.fft as sf

    f = np.ascontiguousarray(x, np.complex64).reshape(-1, 1024)
    if op == "fwd":
        y = sf.fft(f, axis=1)
    elif op == "inv":
        y = sf.ifft(f, axis=1) * np.float32(1024)
    else:
        y = sf.ifft(sf.fft(f, axis=1) * np.asarray(w, np.complex64)[None, :], axis=1) * np.float32(1024)
    assert y.dtype == np.complex64
    return y.ravel()


def launch(op, x, y, nf, w=None, stream=None):
    if op == "chan":
        nsh.channelizer1024(x, y, w, nf, stream=stream)
    else:
        nsh.fft1024(x, y, nf, inverse=(op == "inv"), stream=stream)


def gpu(torch, op, x, w=W, in_off=0, out_off=0, w_off=0, tail=1024):
    """op over x with in / out / w each at a sample offset into a larger allocation; the output
    allocation holds out_off guard samples before the result and `tail` after it. Returns the result
    and checks every guard sample."""
    n = x.size
    dx = torch.zeros(n + 2, dtype=torch.complex64, device="cuda")
    dx[in_off:in_off + n] = dev(torch, x)
    dw = torch.zeros(1024 + 2, dtype=torch.complex64, device="cuda")
    dw[w_off:w_off + 1024] = dev(torch, w)
    dy = torch.full((out_off + n + tail,), GUARD, dtype=torch.complex64, device="cuda")
    launch(op, dx.data_ptr() + 8 * in_off, dy.data_ptr() + 8 * out_off, n // 1024, dw.data_ptr() + 8 * w_off)
    y = host(dy)
    g = np.complex64(GUARD)
    assert np.all(y[:out_off] == g) and np.all(y[out_off + n:] == g), (op, n // 1024, in_off, out_off)
    assert y.size - n == out_off + tail
    return y[out_off:out_off + n]


def report(name, op, y, r, x, w=W):
    """Print err / scale of the kernel and of the fp32 yardstick (reported, not asserted)."""
    ok, err, scale = orc.tol_ok(y, r)
    _, e2, _ = orc.tol_ok(yardstick(op, x, w), r)
    s = scale if scale > 0 else 1.0
    print("RATIO %s %s kernel %.3g scipy_fp32 %.3g" % (name, op, err / s, e2 / s))
    return ok, err, scale


# ---- a. frame counts and the end of the buffer --------------------------------------------------
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("nframes", [1, 2, 3, 4, 5, 7, 8, 9, 37])
def test_frame_counts_and_buffer_end(torch_cuda, op, nframes):
    """Every count that leaves a workgroup's last waves without a frame (and the prefetch of frame
    f + stride past the end): results within tolerance, the 1024 guard samples after them unchanged."""
    x37 = orc.synth(37 * 1024, 100)
    x = x37[: nframes * 1024]
    y = gpu(torch_cuda, op, x)
    ok, err, scale = report("a/nframes=%d" % nframes, op, y, ref(op, x37, key="x37")[: nframes * 1024], x)
    assert ok, (op, nframes, err, scale)


# ---- b. frame independence ----------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_frame_independent_of_batch_and_slot(torch_cuda, op):
    """A frame's output does not depend on its neighbours, its wave slot or the batch size: frames
    0, 1, 3, 4, 35, 36 alone and frames 4..8 as a batch of 5, bit-identical to the batch of 37."""
    x = orc.synth(37 * 1024, 100)
    big = gpu(torch_cuda, op, x)
    for f in (0, 1, 3, 4, 35, 36):
        one = gpu(torch_cuda, op, x[1024 * f:1024 * (f + 1)])
        np.testing.assert_array_equal(bits(one), bits(big[1024 * f:1024 * (f + 1)]), err_msg="frame %d" % f)
    five = gpu(torch_cuda, op, x[1024 * 4:1024 * 9])
    np.testing.assert_array_equal(bits(five), bits(big[1024 * 4:1024 * 9]))


# ---- c. the whole operator on the impulse basis -------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_impulse_basis(torch_cuda, op):
    """1024 frames, frame p a unit impulse at p: the output matrix is the DFT matrix (its conjugate
    for the inverse; the circulant of 1024 ifft(w) for the channelizer). Every element of the DFT
    matrix has modulus 1, so tol_ok bounds each at 1.1e-5 absolute, while a wrong twiddle index,
    digit reversal or pad slip moves one by at least 2 sin(pi / 1024) = 6e-3."""
    x = np.eye(1024, dtype=np.complex64).ravel()
    y = gpu(torch_cuda, op, x)
    r = ref(op, x, key="eye")
    ok, err, scale = report("c/impulses", op, y, r, x)
    assert ok, (op, err, scale)
    if op != "chan":
        pk = (np.arange(1024)[:, None] * np.arange(1024)[None, :]) % 1024
        dft = np.exp((2j if op == "inv" else -2j) * np.pi * pk / 1024).ravel()
        assert np.abs(y - dft).max() <= 1.1e-5


# ---- d. structured frames -----------------------------------------------------------------------
def structured_frames():
    n = np.arange(1024)
    rng = np.random.default_rng(7)
    fr = {"dc": np.full(1024, 0.5 + 0.25j), "nyquist": (-1.0) ** n + 0j}
    for k in (1, 255, 256, 257, 512, 1023):
        fr["tone%d" % k] = np.exp(2j * np.pi * k * n / 1024)  # in double, rounded to complex64 below
    fr["real"] = rng.uniform(-1, 1, 1024) + 0j
    fr["imag"] = 1j * rng.uniform(-1, 1, 1024)
    fr["zero"] = np.zeros(1024, complex)
    return list(fr), np.concatenate([v.astype(np.complex64) for v in fr.values()])


@pytest.mark.parametrize("op", OPS)
def test_structured_frames(torch_cuda, op):
    """DC, Nyquist, single tones, purely real / imaginary and all-zero frames in one batch, each
    within tolerance on its own frame's scale. The DC frame's sums are sums of equal values scaled
    by powers of two, hence exact: bin 0 equals 1024 c. The zero frame's output is exactly zero."""
    names, x = structured_frames()
    y = gpu(torch_cuda, op, x)
    r = ref(op, x, key="structured")
    for i, name in enumerate(names):
        s = slice(1024 * i, 1024 * (i + 1))
        ok, err, scale = report("d/" + name, op, y[s], r[s], x[s])
        assert ok, (op, name, err, scale)
    if op != "chan":
        assert y[0] == np.complex64(1024 * (0.5 + 0.25j))
    z = names.index("zero")
    assert np.all(y[1024 * z:1024 * (z + 1)] == 0)


# ---- e. power-of-two homogeneity ----------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_power_of_two_scaling_is_exact(torch_cuda, op):
    """op(s x) == s op(x) bit for bit for s = 2^-60, 2^60, 2^100 (the channelizer scales x, not w):
    synthetic samples are multiples of 2^-23 in [-1, 1) and the growth is at most 1024 sqrt(2) (times
    |w| <= sqrt(2) and 1024 sqrt(2) again for the channelizer), so nothing under- or overflows."""
    x = orc.synth(5 * 1024, 22)
    y = gpu(torch_cuda, op, x)
    for e in (-60, 60, 100):
        s = np.float32(2.0 ** e)
        ys = gpu(torch_cuda, op, x * s)
        np.testing.assert_array_equal(bits(ys), bits(y * s), err_msg="2^%d" % e)


@pytest.mark.parametrize("op", OPS)
def test_mixed_scales_in_one_batch(torch_cuda, op):
    """Frames at 2^-60, 1 and 2^100 in one batch: each within tolerance on its own scale."""
    x = orc.synth(3 * 1024, 23)
    x[:1024] *= np.float32(2.0 ** -60)
    x[2048:] *= np.float32(2.0 ** 100)
    y = gpu(torch_cuda, op, x)
    r = ref(op, x, key="mixed")
    for f in range(3):
        s = slice(1024 * f, 1024 * (f + 1))
        ok, err, scale = report("e/mixed frame %d" % f, op, y[s], r[s], x[s])
        assert ok, (op, f, err, scale)


# ---- f. non-finite containment ------------------------------------------------------------------
_NAN, _INF = float("nan"), float("inf")


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("bad", [complex(_NAN, _NAN), complex(_INF, 0.0), complex(0.25, -_INF), complex(_NAN, 0.5)],
                         ids=["nan+nanj", "inf+0j", "0.25-infj", "nan+0.5j"])
def test_nonfinite_sample_stays_in_its_frame(torch_cuda, op, bad):
    """One bad sample at index 77 of frame 1 of 3: frames 0 and 2 are bit-identical to the run
    without it, every output of frame 1 is non-finite in at least one part (NaN in both for
    nan+nanj) -- the oracle's mask. Which part is NaN and which inf is left open: it depends on
    where inf * 0 occurs, which differs between this radix-16 kernel and the radix-2 oracle."""
    x = orc.synth(3 * 1024, 21)
    clean = gpu(torch_cuda, op, x)
    xb = x.copy()
    xb[1024 + 77] = bad
    y = gpu(torch_cuda, op, xb)
    for f in (0, 2):
        s = slice(1024 * f, 1024 * (f + 1))
        np.testing.assert_array_equal(bits(y[s]), bits(clean[s]), err_msg="frame %d" % f)
    mid = y[1024:2048]
    nonfinite = ~np.isfinite(mid.real) | ~np.isfinite(mid.imag)
    assert nonfinite.all(), (op, bad, int((~nonfinite).sum()), np.nonzero(~nonfinite)[0][:8].tolist())
    if np.isnan(bad.real) and np.isnan(bad.imag):
        assert np.all(np.isnan(mid.real) & np.isnan(mid.imag))
    r = ref(op, xb)  # the oracle shows the same mask: 0 / 1024 / 0
    rbad = ~np.isfinite(r.real) | ~np.isfinite(r.imag)
    np.testing.assert_array_equal(~np.isfinite(y.real) | ~np.isfinite(y.imag), rbad)


# ---- g. odd sample offsets ----------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_odd_sample_offsets(torch_cuda, op):
    """in, out and w each one complex sample (8 bytes) into a larger allocation, as a flowgraph's
    ring pointers are as often as not: bit-identical to the 16-byte aligned run, the guards before
    and after the output intact (checked in gpu())."""
    x = orc.synth(5 * 1024, 24)
    y0 = gpu(torch_cuda, op, x, out_off=2)  # 16-byte aligned, two guard samples before the output
    combos = [(1, 2, 0), (0, 1, 0), (1, 1, 0), (1, 3, 0)]  # (in, out, w) offsets in samples
    if op == "chan":
        combos += [(0, 2, 1), (1, 1, 1)]
    for in_off, out_off, w_off in combos:
        y = gpu(torch_cuda, op, x, in_off=in_off, out_off=out_off, w_off=w_off)
        np.testing.assert_array_equal(bits(y), bits(y0), err_msg=str((in_off, out_off, w_off)))


# ---- h. channelizer == fft -> multiply_const_vcc -> ifft ----------------------------------------
def weight_sets(golden):
    rng = np.random.default_rng(11)
    special = rand_w(12)
    special[[0, 5, 64, 511]] = 0
    special[[1, 700]] = 1
    special[[2, 701]] = -1
    special[[3, 702]] = 1j
    special[[4, 1023]] = -1j
    special[6] = np.complex64(complex(1e-40, -1e-42))  # subnormal in both parts
    special[7] = np.complex64(complex(0.0, 1e-40))
    return {"golden": golden("fft1024.npz")["w"].astype(np.complex64),
            "random": (rng.standard_normal(1024) + 1j * rng.standard_normal(1024)).astype(np.complex64),
            "special": special}


@pytest.mark.parametrize("wname", ["golden", "random", "special"])
@pytest.mark.parametrize("nframes", [1, 3, 5, 37])
def test_channelizer_equals_staged_kernels(torch_cuda, golden, wname, nframes):
    """The fused channelizer against nsh_fft1024_c2c -> nsh_mul_const_vcc(vlen 1024) ->
    nsh_fft1024_c2c(inverse), bit for bit: the scheduler's channelizer fusion relies on it."""
    torch = torch_cuda
    w = weight_sets(golden)[wname]
    n = nframes * 1024
    x = orc.synth(37 * 1024, 100)[:n]
    fused = gpu(torch, "chan", x, w)
    dx, dw = dev(torch, x), dev(torch, w)
    a, b, c = (torch.empty(n, dtype=torch.complex64, device="cuda") for _ in range(3))
    nsh.fft1024(dx, a, nframes)
    nsh.mul_const_vcc(a, b, dw, 1024, nframes)
    nsh.fft1024(b, c, nframes, inverse=True)
    np.testing.assert_array_equal(bits(fused), bits(host(c)))
    ok, err, scale = report("h/%s nframes=%d" % (wname, nframes), "chan", fused, ref("chan", x, w), x, w)
    assert ok, (wname, nframes, err, scale)


# ---- i. two streams -----------------------------------------------------------------------------
def test_two_streams_back_to_back(torch_cuda):
    """Forward transforms of two different 37-frame inputs on two streams, issued back to back: each
    bit-identical to the same call on the current stream (the twiddle table is shared, per device)."""
    torch = torch_cuda
    xs = [dev(torch, orc.synth(37 * 1024, 100)), dev(torch, orc.synth(37 * 1024, 31))]
    want = [torch.empty_like(x) for x in xs]
    for x, y in zip(xs, want):
        nsh.fft1024(x, y, 37)
    got = [torch.full_like(x, GUARD) for x in xs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for x, y, s in zip(xs, got, streams):
        nsh.fft1024(x, y, 37, stream=s)
    for s in streams:
        s.synchronize()
    for y, r in zip(got, want):
        np.testing.assert_array_equal(bits(host(y)), bits(host(r)))


# ---- j. the armed timing pair -------------------------------------------------------------------
def test_fft_takes_the_armed_timing_pair(torch_cuda):
    """An armed nsh_time_next_launch pair is taken by exactly one launch of nsh_fft1024_c2c, forward
    and inverse (nsh_timed_launches + 1, positive elapsed time); a call with nframes = 0 launches
    nothing and drops the pair, so the next, unarmed launch is not timed."""
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

    nf = 1024
    x = dev(torch, orc.synth(nf * 1024, 11))
    y = torch.empty_like(x)
    for inverse in (False, True):
        ev = events()
        c0 = count()
        assert L.nsh_time_next_launch(ev[0], ev[1]) == 0
        nsh.fft1024(x, y, nf, inverse=inverse)
        assert count() == c0 + 1
        nsh.fft1024(x, y, nf, inverse=inverse)  # unarmed: not counted
        assert count() == c0 + 1
        torch.cuda.synchronize()
        ms = C.c_float()
        assert L.nsh_event_elapsed_ms(ev[0], ev[1], C.byref(ms)) == 0 and ms.value > 0
        for e in ev:
            L.nsh_event_destroy(e)
    ev = events()
    c0 = count()
    assert L.nsh_time_next_launch(ev[0], ev[1]) == 0
    nsh.fft1024(x, y, 0)   # nothing to do: no launch, the pair is dropped on return
    nsh.fft1024(x, y, nf)  # unarmed
    torch.cuda.synchronize()
    assert count() == c0
    ms = C.c_float()
    assert L.nsh_event_elapsed_ms(ev[0], ev[1], C.byref(ms)) != 0  # never recorded
    for e in ev:
        L.nsh_event_destroy(e)
