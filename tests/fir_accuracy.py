"""What tests/test_gpu_fir_accuracy.py judges the time-domain kernels by: fft_accuracy's two figures
(rms error of the whole call and of its worst position, over the rms of the reference) held to a
small factor of the same figures of an fp32 model that sums in the order the kernel's header documents.

References: the float64 definitions on the same fp32 inputs (xlat_ref, resamp_ref, arb_ref, pfb_ref,
synth_ref; fir_ref is xlat_ref untuned), the one copy the GPU tests of each block import. resamp_ref and
pfb_ref are polyphase sums; resamp_ref_conv and pfb_ref_conv are the same outputs by np.convolve
straight from the definition, and test_cpu_references_agree holds each pair together.
tests/test_gpu_stream_forms.py takes its fp32 emulation from here, and the plan geometry it shares
with the CPU layout tests (the stream forms, below).

Models: numpy, fp32 values carried in float64 arrays. One FMA is fl32(a b + c) with the product exact
in double (_fma32's rule). Every model takes the switches of the CPU tests: fma=False rounds the
product before the add (a second correct implementation), the others plant one defect each.
  fir_model        k_fir_direct: taps k ascending, one FMA per term (nsh_fir.hip: "fp32 accumulation in
                   tap order"; it documents no blocking of the sum).
  xlat_model       k_fir_xlat: samples rotated once and rounded to fp32 (rotate_stream), reversed taps q
                   ascending per wave part, the S parts "added in part order" (nsh_xlat.hip).
  rotate_stream    the phasor of nsh_phase.hpp: the top 32 phase bits as a signed fp32 number of
                   half-turns, cos / sin rounded once; the second sample of a 16-byte pair takes the
                   first's phasor times the fp32 step phasor; a rotation is one rounded product and
                   one FMA per component (crot).
  resamp_model     k_resamp: q ascending, one FMA per term.
  arb_model        k_arb: w = fl32(mu d + h) (one FMA), mu from the top 24 fraction bits, q ascending.
  pfb_model        k_pfb: the branch sums q ascending, then the header's radix-2 decimation in frequency
  synth_model      over the M lanes (dif_network: a +- b, then one rounded product and one FMA per
                   component with the table rounded once from double; no twiddle in the last stage);
                   k_pfb_synth runs the network first and the branch FIRs after it.
  f32mfma_model    k_fir_f32mfma and the exact tile the split kernels fall back to: fp32 products, an
                   fmaf chain over tap blocks q, steps s and k = lane group g of each 16x16x4 MFMA
                   (sample 4 g + s of the block: nsh_fir_f32.hip).
  mfma12_model     the fp16x2 split of nsh_fir_mfma_shared.hpp: taps scaled to [2^14, 2^15) and split
  decim_model      hi / lo RNE, samples scaled per 2048-sample chunk from the largest magnitude of the
                   chunk and its halo (pred=True: the chunk and its whole predecessor, k_fir_mfma11),
                   split hi / lo RNE; x0h0 into one fp32 accumulator, x0h1 then x1h0 into a second, MFMA
                   by MFMA in the kernels' k order (k_fir_mfma12: 16 samples a step, newest block
                   first; the decimators: phase by phase, 32 samples a step, the odd block into
                   accumulators of its own), the accumulators added and unscaled. Inside one MFMA the
                   hardware's order is not documented: group=16 sums each MFMA's 16 (32) terms in
                   groups of 16 exactly and rounds once per group, group=4 in groups of 4.

Positions: an output's place in the unit the kernel repeats (positions_* below).

The factors. Measured on the CPU by test_cpu_* of tests/test_gpu_fir_accuracy.py (127 taps where
the family takes them, uniform data, at least 64 frames and 2^16 outputs; kernel / model as the
gate forms it, against each family's model; whole, worst):
  correct implementations
    the product rounded before the add         1.016 .. 1.083   0.983 .. 1.107   the nine families with an FMA
    every sample's own phasor, rounded once    0.933 .. 0.992   0.837 .. 1.034   k_rotate, k_fir_xlat
    fp16x2, groups of 16 against groups of 4   0.668 .. 0.751   0.620 .. 0.755   k_fir_mfma12, 13<2>, 13<4>
    fp16x2, groups of 8 against groups of 4    0.792 .. 0.837   0.746 .. 0.843   (where the hardware was found)
  defects
    one dominant tap x (1 + 1e-6)              1.67 .. 7.65     1.60 .. 6.26     smallest: k_pfb 1.67, 1.60; k_pfb_synth
                                                                                 1.67, 5.91; k_fir_xlat 1.92, 1.75
    the taps' low fp16 term dropped            1129 .. 1714     907 .. 1588
    the split truncates both terms             2.51 .. 4.00     2.39 .. 3.07
    phasor from the top 24 phase bits          1.74, 3.72       1.62, 3.16       k_fir_xlat, k_rotate
    mu from the top 16 fraction bits           12.9             12.8
    one DFT table entry x (1 + 1e-6)           1.62, 1.60       2.05, 1.73       k_pfb, k_pfb_synth
The correct implementations reach 1.083 and 1.107, the smallest defect gives 1.60 in whole (and 1.60 in
worst): WHOLE = 1.25 and WORST = 1.5, the FFT family's, lie between in every family.
Not visible to this gate, inside the correct spread (test_cpu_defects_fail keeps the list true):
    the split's low terms truncated, not RNE   0.638 .. 0.744   0.651 .. 0.744   the 16-term model's own figures:
                                                                                 part 3's bound is for this one
    k_fir_direct's sum with k descending       0.997            0.896            not worse orders: no plausible
    ... even taps, then odd taps               0.999            0.903            worse one was found
The fp16x2 kernels are gated against the 4-term grouping, the loosest of the three models; the
hardware's own (8 terms: one lane's operand of the MFMA) is printed beside it.
"""
import math

import numpy as np

from oracle import oracle as orc
from tests import fft_accuracy as fa
from tests.fft_accuracy import MIN_FRAMES, MIN_OUTPUTS, frames_for, stats  # noqa: F401  (re-exported)
from tests.gpu_util import dev, first_mismatch, host, int_signal, int_taps  # noqa: F401  (dev: re-exported)

WHOLE, WORST = 1.25, 1.5


def gate(name, y, model, r, frames):
    """fft_accuracy.gate (the same two conditions on frames and outputs) at the FIR family's factors."""
    return fa.gate(name, y, model, r, frames, whole=WHOLE, worst=WORST)


def ratios(y, model, r, frames):
    """(whole ratio, worst ratio) of y against the model, as gate() forms them, without asserting."""
    wk, pk = stats(y, r, frames)
    wm, pm = stats(model, r, frames)
    return wk / wm, pk / pm


def ceil_div(a, b):
    return -(-a // b)


# ---- the references, float64, per output ------------------------------------------------------------
# hist = the samples before x[0], or None for zeros. Non-finite samples are data here (the tests that
# plant a NaN or an Inf read where it lands), so the sums run with numpy's warnings off.
def _ext(hist, H, x):
    """[hist | x] in complex128, H zeros where hist is None."""
    h0 = np.zeros(H, np.complex128) if hist is None else hist.astype(np.complex128)
    return np.concatenate([h0, x.astype(np.complex128)])


def phasors(first, n, inc):
    idx = (np.uint64(first % 2 ** 64) + np.arange(n, dtype=np.uint64))      # wraps mod 2^64
    p = idx * np.uint64(inc)
    turns = (p >> np.uint64(11)).astype(np.float64) / 2.0 ** 53
    return np.exp(2j * np.pi * turns)


def xlat_ref(x, hist, taps, D, inc, first, n_out):
    """y[m] = sum_k h[k] rot(x)[mD - k]; hist = the L-1 raw samples before x[0]."""
    L = len(taps)
    ext = _ext(hist, L - 1, x)
    with np.errstate(invalid="ignore", over="ignore"):
        ext = ext * phasors(first - (L - 1), ext.size, inc)
        full = np.convolve(ext, np.asarray(taps, np.float64))
    return full[L - 1::D][:n_out]


def xlat_ref_at(x, hist, taps, D, inc, first, n_out):
    """xlat_ref's definition evaluated at the n_out decimated outputs alone, tap by tap in float64 (the
    full-rate convolution of 2^16 D samples with 1024 taps takes a minute at D = 64).
    test_cpu_references_agree holds the two together."""
    L = len(taps)
    ext = _ext(None if hist is None else hist[:L - 1], L - 1, x)
    if inc:
        with np.errstate(over="ignore"):
            ext = ext * phasors(first - (L - 1), ext.size, inc)
    h = np.asarray(taps, np.float64)
    y = np.zeros(n_out, np.complex128)
    for k in range(L):
        y += h[k] * ext[L - 1 - k:L - 1 - k + (n_out - 1) * D + 1:D]
    return y


def fir_ref(x, hist, taps, D, n_out):
    """y[m] = sum_k h[k] x[mD - k]: the xlating reference untuned."""
    return xlat_ref_at(x, hist, taps, D, 0, 0, n_out)


def rotate_ref(x, inc, first):
    with np.errstate(over="ignore"):
        return x.astype(np.complex128) * phasors(first, x.size, inc)


def resamp_ref(x, hist, taps, I, D, n_units):
    """The polyphase sum: y[n] = sum_q h[phi + q I] x[j0 - q], phi = (n D) mod I, j0 = floor(n D / I);
    hist = the Q-1 samples before x[0]."""
    L = len(taps)
    Q = ceil_div(L, I)
    H = Q - 1
    ext = _ext(hist, H, x[:n_units * D])
    h = np.zeros(Q * I)
    h[:L] = taps
    n = np.arange(n_units * I)
    j0, phi = n * D // I, n * D % I
    y = np.zeros(n.size, np.complex128)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(Q):
            y += h[phi + q * I] * ext[H + j0 - q]
    return y


def resamp_ref_conv(x, hist, taps, I, D, n_units):
    """The same from the definition: stuff I - 1 zeros between the samples, filter, keep every D-th."""
    L = len(taps)
    H = ceil_div(L, I) - 1
    ext = _ext(hist, H, x[:n_units * D])
    u = np.zeros(ext.size * I, np.complex128)
    u[::I] = ext
    return np.convolve(u, np.asarray(taps, np.float64))[H * I::D][:n_units * I]


def arb_indices(step, F, phase, n_out):
    """i, j (int64) and mu (float32, as the kernel forms it) of the outputs 0 .. n_out-1. Positions in
    Python integers: no phase or step wraps."""
    pos = [phase + n * step for n in range(n_out)]
    k = np.array([p >> 32 for p in pos], np.int64)
    frac = np.array([p & 0xffffffff for p in pos], np.uint32)
    mu = (frac >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return k // F, k % F, mu


def diff_taps(taps):
    t = np.asarray(taps, np.float32)
    return np.concatenate([t[1:] - t[:-1], np.zeros(1, np.float32)]).astype(np.float32)


def arb_ref(x, hist, taps, F, step, phase, n_out):
    """y[n] = sum_q (h[j + q F] + mu d[j + q F]) x[i - q] over j + q F < L; hist = the Q-1 samples before x[0]."""
    L = len(taps)
    Q = ceil_div(L, F)
    H = Q - 1
    i, j, mu = arb_indices(step, F, phase, n_out)
    assert i.max() < x.size
    ext = _ext(hist, H, x)
    h = np.asarray(taps, np.float64)
    d = diff_taps(taps).astype(np.float64)
    mu = mu.astype(np.float64)
    y = np.zeros(n_out, np.complex128)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(Q):
            t = j + q * F
            tc = np.minimum(t, L - 1)
            y += np.where(t < L, (h[tc] + mu * d[tc]) * ext[i - q + H], 0)
    return y


def pfb_ref(x, hist, taps, M, n_out):
    """The polyphase sum, (n_out, M): y[m][c] = sum_p u_p[m] exp(2j pi c p / M),
    u_p[m] = sum_q h[p + q M] x[(m - q) M - p]; hist = the L-1 samples before x[0]. Channels 0 and M/2
    are the plain and the alternating sum of the branches: exact on integer data."""
    L = len(taps)
    Q = ceil_div(L, M)
    ext = np.concatenate([np.zeros(Q * M, np.complex128), _ext(hist, L - 1, x)])
    at0 = Q * M + L - 1                                   # x[0]
    h = np.zeros(Q * M)
    h[:L] = taps
    m, p = np.arange(n_out)[:, None], np.arange(M)[None, :]
    u = np.zeros((n_out, M), np.complex128)
    c = np.arange(M)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(Q):
            u += h[p + q * M] * ext[at0 + (m - q) * M - p]
        y = u @ np.exp(2j * np.pi * ((p.T * c[None, :]) % M) / M)
        y[:, 0] = u.sum(axis=1)
        y[:, M // 2] = (u * (1 - 2 * (p % 2))).sum(axis=1)
    return y


def pfb_ref_conv(x, hist, taps, M, n_out):
    """The same from the definition, (n_out, M): channel c is the stream filtered by
    h[k] exp(2j pi c k / M) and decimated by M."""
    L = len(taps)
    ext = _ext(hist, L - 1, x)
    k = np.arange(L)
    y = np.empty((n_out, M), np.complex128)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(M):
            hc = np.asarray(taps, np.float64) * np.exp(2j * np.pi * ((c * k) % M) / M)
            y[:, c] = np.convolve(ext, hc)[L - 1::M][:n_out]
    return y


def synth_ref(x, hist, taps, M):
    """The synthesizer's polyphase model, n M outputs: v[m] = M ifft(X[m]) over the channels of every
    item, y[m M + r] = sum_q h[r + q M] v_r[m - q]. x: n items of M, flat or (n, M); hist: the Q-1
    items before them, flat or (Q-1, M), None or empty = zeros."""
    L = len(taps)
    Q = ceil_div(L, M)
    hp = np.zeros(Q * M)
    hp[:L] = taps
    X = x.reshape(-1, M)
    h0 = np.zeros((Q - 1, M), np.complex128) if hist is None or not hist.size else hist.reshape(Q - 1, M)
    ext = np.concatenate([h0, X]).astype(np.complex128)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.fft.ifft(ext, axis=1) * M
        y = np.zeros((X.shape[0], M), np.complex128)
        for q in range(Q):
            y += hp[q * M:(q + 1) * M][None, :] * v[Q - 1 - q:Q - 1 - q + X.shape[0]]
    return y.reshape(-1)


# ---- fp32 arithmetic in numpy -------------------------------------------------------------------------
def _fma32(a, b, acc):
    """fl32(a b + acc) for fp32 a, b, acc: the product is exact in double, one further rounding."""
    return (a.astype(np.float64) * b.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def _emulate(w, xw):
    """Row-wise fp32 sums of w[:, q] xw[:, q], q ascending, one FMA per component and term."""
    re = np.zeros(xw.shape[0], np.float32)
    im = np.zeros(xw.shape[0], np.float32)
    xr, xi = np.ascontiguousarray(xw.real), np.ascontiguousarray(xw.imag)
    for q in range(xw.shape[1]):
        re = _fma32(w[:, q], xr[:, q], re)
        im = _fma32(w[:, q], xi[:, q], im)
    return re + 1j * im.astype(np.float64)


def _r32(a):
    """Round to fp32, carried on in float64."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _planes(z):
    """A complex array as (2, n) float64: re and im of fp32 values."""
    z = np.asarray(z)
    return np.stack([z.real, z.imag]).astype(np.float64)


def _cplx(p):
    return p[0] + 1j * p[1]


def _mac(w, x, acc, fma=True):
    """acc + w x in fp32 (values in float64): one FMA, or a rounded product and a rounded add."""
    return _r32(w * x + acc) if fma else _r32(_r32(w * x) + acc)


def _f32(taps):
    return np.asarray(taps, np.float32).astype(np.float64)


# ---- k_fir_direct -------------------------------------------------------------------------------------
def fir_model(x, hist, taps, D, n_out, fma=True, order=None):
    """Taps in the order k = 0 .. L-1 (order: another permutation of them), one FMA per term."""
    L = len(taps)
    ext = _planes(np.concatenate([hist[:L - 1], x]))
    h = _f32(taps)
    acc = np.zeros((2, n_out))
    for k in (range(L) if order is None else order):
        s = L - 1 - k
        acc = _mac(h[k], ext[:, s:s + (n_out - 1) * D + 1:D], acc, fma)
    return _cplx(acc)


# ---- the phasor, k_rotate and k_fir_xlat --------------------------------------------------------------
def phasor_top(p, bits=32):
    """(cos, sin), fp32, of the phase p (uint64) from its top 32 bits as nsh::phasor takes them: a signed
    number of half-turns rounded to fp32, cos / sin rounded once. bits < 32: the lower ones cleared first."""
    s = (p >> np.uint64(32)).astype(np.uint32)
    if bits < 32:
        s = s & np.uint32((0xffffffff << (32 - bits)) & 0xffffffff)
    v = s.view(np.int32).astype(np.float32).astype(np.float64) * 2.0 ** -31
    return _r32(np.cos(np.pi * v)), _r32(np.sin(np.pi * v))


def step_phasor(inc):
    """exp(j 2 pi inc / 2^64), the short way round, in double and rounded to fp32 (nsh_xlat.hip)."""
    signed = inc - 2 ** 64 if inc >= 2 ** 63 else inc
    th = 2.0 * math.pi * math.ldexp(float(signed), -64)
    return float(np.float32(math.cos(th))), float(np.float32(math.sin(th)))


def crot32(ar, ai, wr, wi, fma=True):
    """nsh::crot: a w with one rounded product and one FMA per component."""
    if fma:
        return _r32(-ai * wi + _r32(ar * wr)), _r32(ar * wi + _r32(ai * wr))
    return _r32(_r32(ar * wr) - _r32(ai * wi)), _r32(_r32(ar * wi) + _r32(ai * wr))


def rotate_stream(raw, idx0, inc, bits=32, pair=True, fma=True):
    """(re, im), fp32, of raw[i] exp(j 2 pi phase(idx0 + i)). Even i: the phasor of the sample's own
    phase; odd i: the phasor of i - 1 times the step phasor (pair=False: its own, the exactly rounded
    alternative)."""
    n = raw.size
    i = np.arange(n, dtype=np.uint64)
    src = (i & ~np.uint64(1)) if pair else i
    with np.errstate(over="ignore"):
        p = (np.full(1, idx0 % 2 ** 64, np.uint64) + src) * np.full(1, inc, np.uint64)
    c, s = phasor_top(p, bits)
    if pair:
        sc, ss = step_phasor(inc)
        c2, s2 = crot32(c, s, sc, ss)
        odd = (i & np.uint64(1)) == 1
        c, s = np.where(odd, c2, c), np.where(odd, s2, s)
    z = _planes(raw)
    return crot32(z[0], z[1], c, s, fma)


def rotate_model(x, inc, first, **kw):
    return _cplx(rotate_stream(x, first, inc, **kw))


def xlat_model(x, hist, taps, D, inc, first, n_out, fma=True, **rot):
    """Window position i of a workgroup is stream sample m0 D - (L-1) + i with m0 D even: pairs are even
    and odd positions of hist ++ x. Reversed taps g[q] = h[L-1-q] in S parts of Lc, a multiple of 8."""
    L = len(taps)
    S = xlat_form(D)[1]
    Lc = ceil_div(ceil_div(L, S), 8) * 8
    ext = np.stack(rotate_stream(np.concatenate([hist[:L - 1], x]), first - (L - 1), inc, **rot))
    g = _f32(taps)[::-1]
    total = None
    for part in range(S):
        acc = np.zeros((2, n_out))
        for q in range(part * Lc, min(L, part * Lc + Lc)):
            acc = _mac(g[q], ext[:, q:q + (n_out - 1) * D + 1:D], acc, fma)
        total = acc if total is None else _r32(total + acc)
    return _cplx(total)


# ---- k_resamp, k_arb ----------------------------------------------------------------------------------
def resamp_model(x, hist, taps, I, D, n_units, fma=True):
    L = len(taps)
    Q = ceil_div(L, I)
    H = Q - 1
    ext = _planes(np.concatenate([hist[:H], x[:n_units * D]]))
    h = np.zeros(Q * I)
    h[:L] = _f32(taps)
    n = np.arange(n_units * I)
    j0, phi = n * D // I, n * D % I
    acc = np.zeros((2, n.size))
    for q in range(Q):
        acc = _mac(h[phi + q * I], ext[:, H + j0 - q], acc, fma)
    return _cplx(acc)


def arb_model(x, hist, taps, F, step, phase, n_out, fma=True, mu_bits=24):
    """w = fl32(mu d + h) and acc = fl32(w x + acc), q ascending. mu_bits < 24: mu cut to its top bits."""
    L = len(taps)
    Q = ceil_div(L, F)
    H = Q - 1
    i, j, mu = arb_indices(step, F, phase, n_out)
    mu = mu.astype(np.float64)
    if mu_bits < 24:
        mu = np.floor(mu * 2.0 ** mu_bits) / 2.0 ** mu_bits
    ext = _planes(np.concatenate([hist[:H], x]))
    h, d = _f32(taps), diff_taps(taps).astype(np.float64)
    acc = np.zeros((2, n_out))
    for q in range(Q):
        t = j + q * F
        tc = np.minimum(t, L - 1)
        w = np.where(t < L, _mac(mu, d[tc], h[tc], fma), 0.0)
        acc = _mac(w, ext[:, i - q + H], acc, fma)
    return _cplx(acc)


# ---- k_pfb, k_pfb_synth ---------------------------------------------------------------------------------
def pfb_tables(M):
    """tw[s][lane], s < log2 M - 1 (nsh_pfb_geom.hpp): 1 for the lane without the stage's bit,
    exp(+j 2 pi (lane mod half) / (2 half)) for the one with it, the quadrant points exact, rounded once."""
    tables = []
    for s in range(M.bit_length() - 2):
        half = M >> (s + 1)
        q = np.arange(M)
        i = q & (half - 1)
        th = 2.0 * np.pi * i / (2 * half)
        c, sn = np.cos(th), np.sin(th)
        c[4 * i == 2 * half], sn[4 * i == 2 * half] = 0.0, 1.0
        on = (q & half) != 0
        tables.append((_r32(np.where(on, c, 1.0)), _r32(np.where(on, sn, 0.0))))
    return tables


def dif_network(ur, ui, tables=None, fma=True):
    """k_pfb's inverse DFT across the last axis (M lanes): log2 M stages of one exchange with lane ^ half;
    the lane without the bit keeps a + b, the one with it (a_low - a_high) w; lane p ends with element
    bitrev(p). Returns natural order."""
    M = ur.shape[-1]
    stages = M.bit_length() - 1
    tables = pfb_tables(M) if tables is None else tables
    p = np.arange(M)
    for s in range(stages):
        half = M >> (s + 1)
        sgn = np.where(p & half, -1.0, 1.0)
        tr, ti = _r32(ur * sgn + ur[..., p ^ half]), _r32(ui * sgn + ui[..., p ^ half])
        if s < stages - 1:
            ur, ui = crot32(tr, ti, tables[s][0], tables[s][1], fma)
        else:
            ur, ui = tr, ti
    rev = np.zeros(M, np.int64)
    for b in range(stages):
        rev |= ((p >> b) & 1) << (stages - 1 - b)
    outr, outi = np.empty_like(ur), np.empty_like(ui)
    outr[..., rev], outi[..., rev] = ur, ui
    return outr, outi


def pfb_model(x, hist, taps, M, n_out, fma=True, tables=None):
    """(n_out, M). Branch p: u_p[m] = sum_q h[p + q M] x[(m - q) M - p], q ascending; then dif_network."""
    L = len(taps)
    Q = ceil_div(L, M)
    ext = _planes(np.concatenate([np.zeros(Q * M, np.complex64), hist[:L - 1], x]))
    at0 = Q * M + L - 1
    h = np.zeros(Q * M)
    h[:L] = _f32(taps)
    m, p = np.arange(n_out)[:, None], np.arange(M)[None, :]
    acc = np.zeros((2, n_out, M))
    for q in range(Q):
        acc = _mac(h[p + q * M], ext[:, at0 + (m - q) * M - p], acc, fma)
    return _cplx(dif_network(acc[0], acc[1], tables, fma))


def synth_model(x, hist, taps, M, fma=True, tables=None):
    """Flat n M outputs. v_r[m] by dif_network over the channels of every item (the Q-1 history items
    too), then y[m M + r] = sum_q h[r + q M] v_r[m - q], q ascending."""
    L = len(taps)
    Q = ceil_div(L, M)
    items = np.concatenate([hist[:(Q - 1) * M], x]).reshape(-1, M)
    z = _planes(items)
    v = np.stack(dif_network(z[0], z[1], tables, fma))
    n = items.shape[0] - (Q - 1)
    h = np.zeros(Q * M)
    h[:L] = _f32(taps)
    acc = np.zeros((2, n, M))
    for q in range(Q):
        acc = _mac(h[q * M:(q + 1) * M][None, :], v[:, Q - 1 - q:Q - 1 - q + n], acc, fma)
    return _cplx(acc).reshape(-1)


# ---- the exact-fp32 matrix tile -------------------------------------------------------------------------
def f32mfma_model(x, hist, taps, n_out, QF=None, fma=True):
    """y[16 beta + j] = sum_q sum_s sum_g h[j - r + 16 q] x[16 (beta - q) + r], r = 4 g + s: tap blocks q
    ascending, the four MFMAs s of a block in turn, k = g ascending inside one (an fmaf chain, one
    rounding per term). QF tap blocks of 16: k_fir_f32mfma's (L + 30) / 16 unless given (the split
    kernels' exact tile: 2 Q - 1)."""
    L = len(taps)
    QF = (L + 30) // 16 if QF is None else QF
    assert L - 1 <= 16 * (QF - 1)
    ext = _planes(np.concatenate([np.zeros(16 * QF, np.complex64), hist[:L - 1], x]))
    at0 = 16 * QF + L - 1
    h = _f32(taps)
    n = np.arange(n_out)
    beta, j = n >> 4, n & 15
    acc = np.zeros((2, n_out))
    for q in range(QF):
        for s in range(4):
            for g in range(4):
                r = 4 * g + s
                k = j - r + 16 * q
                ok = (k >= 0) & (k < L)
                if not ok.any():
                    continue
                w = np.where(ok, h[np.clip(k, 0, L - 1)], 0.0)
                acc = _mac(w, ext[:, at0 + 16 * (beta - q) + r], acc, fma)
    return _cplx(acc)


# ---- the fp16x2 split -------------------------------------------------------------------------------------
def scale_exp(maxabs):
    """scale_of: 141 - the biased exponent of the largest magnitude, so that it scales into [2^14, 2^15)."""
    return 141 - int(np.float32(maxabs).view(np.uint32) >> np.uint32(23))


def split16(v, trunc=False):
    """v (fp32 values) -> (hi, lo), fp16 values in float64: hi = RNE fp16 of v, lo = RNE fp16 of the exact
    residual. Defects: trunc=True rounds both toward zero instead, trunc="lo" the low term alone."""
    def to16(a, trunc):
        with np.errstate(over="ignore"):
            h = a.astype(np.float32).astype(np.float16)
        if trunc:
            over = np.abs(h.astype(np.float64)) > np.abs(a)
            h = np.where(over, np.nextafter(h, np.float16(0)), h)
        return h.astype(np.float64)

    hi = to16(v, trunc is True)
    return hi, to16(v - hi, bool(trunc))


def tap_split(taps, drop_lo=False, trunc=False):
    """(sh, h0, h1): max |h| 2^sh in [2^14, 2^15), the scaled taps split hi / lo."""
    h = _f32(taps)
    sh = scale_exp(np.max(np.abs(h)))
    h0, h1 = split16(np.ldexp(h, sh), trunc)
    return sh, h0, (np.zeros_like(h1) if drop_lo else h1)


def chunk_scales(ext, at0, n_in, halo, pred=False, scale_off=0):
    """The scale exponent of every 2048-sample chunk of the call: from the largest component magnitude
    of the chunk and the `halo` samples before it (pred: the whole chunk before it)."""
    mag = np.max(np.abs(ext), axis=0)
    back = 2048 if pred else halo
    return np.array([scale_exp(mag[max(at0 + 2048 * c - back, 0):at0 + 2048 * (c + 1)].max()) + scale_off
                     for c in range(ceil_div(n_in, 2048))])


class _Split:
    """The call's samples scaled by their output's chunk scale and split: of(idx) -> (x0, x1) planes for
    ext positions idx (one per output). One split of the whole stream where every chunk has one scale."""

    def __init__(self, ext, sc, trunc):
        self.ext, self.sc, self.trunc = ext, sc, trunc
        self.whole = split16(np.ldexp(ext, int(sc[0])), trunc) if np.all(sc == sc[0]) else None

    def of(self, idx):
        if self.whole is not None:
            return self.whole[0][:, idx], self.whole[1][:, idx]
        return split16(np.ldexp(self.ext[:, idx], self.sc[None, :]), self.trunc)


def _mfma(terms, group):
    """One MFMA's K terms (None or (x0h0, x0h1, x1h0), each exact in double) in groups of `group`
    consecutive k: three lists of exact group sums."""
    out = ([], [], [])
    for a in range(0, len(terms), group):
        live = [t for t in terms[a:a + group] if t is not None]
        if live:
            for i in range(3):
                out[i].append(sum(t[i] for t in live))
    return out


def _acc3(hi, lo, parts):
    """acc_hi += x0h0; acc_lo += x0h1; acc_lo += x1h0: one rounding per group."""
    for g in parts[0]:
        hi = _r32(hi + g)
    for g in parts[1]:
        lo = _r32(lo + g)
    for g in parts[2]:
        lo = _r32(lo + g)
    return hi, lo


def _term(sp, h0, h1, k, idx):
    L = h0.size
    ok = (k >= 0) & (k < L)
    if not ok.any():
        return None
    kc = np.clip(k, 0, L - 1)
    a0, a1 = np.where(ok, h0[kc], 0.0), np.where(ok, h1[kc], 0.0)
    x0, x1 = sp.of(idx)
    return x0 * a0, x0 * a1, x1 * a0


def mfma12_model(x, hist, taps, n_out, group=16, drop_lo=False, trunc=False, scale_off=0, unscale_off=0):
    """k_fir_mfma12: y[32 beta + i] = sum_q sum_r h[i - r + 32 q] x[32 (beta - q) + r], 2 Q steps of 16
    samples (block q = step / 2, its first half, then its second)."""
    L = len(taps)
    Q = (L + 30) // 32 + 1
    ext = _planes(np.concatenate([np.zeros(32 * Q, np.complex64), hist[:L - 1], x]))
    at0 = 32 * Q + L - 1
    sh, h0, h1 = tap_split(taps, drop_lo, trunc)
    n = np.arange(n_out)
    sc = chunk_scales(ext, at0, n_out, 32 * (Q - 1), False, scale_off)[n >> 11]
    sp = _Split(ext, sc, trunc)
    beta, i = n >> 5, n & 31
    hi, lo = np.zeros((2, n_out)), np.zeros((2, n_out))
    for st in range(2 * Q):
        q = st >> 1
        terms = [_term(sp, h0, h1, i - r + 32 * q, at0 + 32 * (beta - q) + r) for r in range(16 * (st & 1), 16 * (st & 1) + 16)]
        hi, lo = _acc3(hi, lo, _mfma(terms, group))
    return _cplx(_r32(np.ldexp(_r32(hi + lo), -(sc + sh) + unscale_off)))


def decim_qh(L, D):
    return (ceil_div(L, D) + 31) // 16


def decim_model(x, hist, taps, D, n_out, group=16, pred=False, drop_lo=False, trunc=False, scale_off=0, unscale_off=0):
    """k_fir_mfma13 (pred: k_fir_mfma11's scale) on the phase streams z_0[i] = x[D i], z_r[i] = x[D i + D - r]:
    y[16 beta + i] = sum_r sum_q sum_rho h'_r[i - rho + 16 q] z_r[16 (beta - q) + rho]. Phase by phase,
    QH / 2 MFMAs of two blocks (k < 16: block 2 st, then block 2 st + 1), the odd last block into
    accumulators of its own; (hi + hi_t) + (lo + lo_t), unscaled."""
    L = len(taps)
    QH = decim_qh(L, D)
    KS, TAIL = QH // 2, QH % 2
    pad = 16 * QH * D
    ext = _planes(np.concatenate([np.zeros(pad, np.complex64), hist[:L - 1], x]))
    at0 = pad + L - 1
    sh, h0, h1 = tap_split(taps, drop_lo, trunc)
    m = np.arange(n_out)
    sc = chunk_scales(ext, at0, n_out * D, D * 16 * (QH - 1), pred, scale_off)[(m * D) >> 11]
    sp = _Split(ext, sc, trunc)
    beta, i = m >> 4, m & 15
    z = np.zeros((2, n_out))
    hi, lo, hi_t, lo_t = z, z.copy(), z.copy(), z.copy()

    def term(r, q, rho):
        sr = 0 if r == 0 else D - r
        return _term(sp, h0, h1, D * (i - rho + 16 * q) - sr, at0 + D * (16 * (beta - q) + rho) + sr)

    for r in range(D):
        for st in range(KS):
            terms = [term(r, 2 * st + (k >> 4), k & 15) for k in range(32)]
            hi, lo = _acc3(hi, lo, _mfma(terms, group))
        if TAIL:
            terms = [term(r, QH - 1, k) for k in range(16)]
            hi_t, lo_t = _acc3(hi_t, lo_t, _mfma(terms, group))
    s = _r32(_r32(hi + hi_t) + _r32(lo + lo_t))
    return _cplx(_r32(np.ldexp(s, -(sc + sh) + unscale_off)))


def split_bound(x, taps, D, n_out, halo):
    """The header's per-component bound of an L <= 2 filter on the split path (part 3 of the gate's issue):
    per term 4 2^-22 |x h| + 2^-38 max|chunk| max|h| (the dropped x1h1, one 2^-22 for each operand's
    split, two fp32 roundings; the subnormal low term's floor 2^-39, doubled), one more rounding
    2^-24 sum |x h| for the second term. x: hist ++ samples with L - 1 history samples, as the models
    take them. Returns (2, n_out)."""
    L = len(taps)
    assert L <= 2
    ext = _planes(x)
    h = _f32(taps)
    mag = np.max(np.abs(ext), axis=0)
    n_in = n_out * D
    cmax = np.array([mag[max(L - 1 + 2048 * c - halo, 0):L - 1 + 2048 * (c + 1)].max() for c in range(ceil_div(n_in, 2048))])
    floor = 2.0 ** -38 * cmax[(np.arange(n_out) * D) >> 11] * np.max(np.abs(h))
    terms = [np.abs(h[k] * ext[:, L - 1 - k:L - 1 - k + (n_out - 1) * D + 1:D]) for k in range(L)]
    b = sum(4 * 2.0 ** -22 * t + floor[None, :] for t in terms)
    return b + (2.0 ** -24 * sum(terms) if L == 2 else 0.0)


# ---- the FIR kernels' dispatch, restated (tests/test_gpu_fir_forms.py pins the lists) ----------------
MAX_TAPS = 4096


def q12(L):
    return (L + 30) // 32 + 1


def qf(L):
    return (L + 30) // 16


def fir_bucket_ends(bucket, supported):
    """Smallest and largest L of every bucket among the tap counts the form accepts."""
    ends = {}
    for L in range(1, MAX_TAPS + 1):
        if supported(L):
            lo, hi = ends.get(bucket(L), (L, L))
            ends[bucket(L)] = (min(lo, L), max(hi, L))
    return sorted({L for lo_hi in ends.values() for L in lo_hi})


ENDS_12 = fir_bucket_ends(q12, lambda L: q12(L) <= 6)
ENDS_D = {D: fir_bucket_ends(lambda L, D=D: decim_qh(L, D), lambda L, D=D: decim_qh(L, D) <= 6) for D in (2, 4)}
ENDS_F32 = fir_bucket_ends(qf, lambda L: qf(L) <= 17)
DIRECT_R = {1: 8, 2: 8, 4: 4, 8: 2}
# the first tap count past each matrix form's range: AUTO switches to the direct form there
AUTO_DIRECT = {1: ENDS_12[-1] + 1, 2: ENDS_D[2][-1] + 1, 4: ENDS_D[4][-1] + 1}


def direct_name(D):
    return "k_fir_direct<%d,%d>" % (D, DIRECT_R[D])


# ---- the stream kernels' dispatch, restated (tests/test_gpu_stream_forms.py pins the lists) ----------
# k_fir_xlat<R,S>
XLAT_BUCKETS = [(4, 8, 1), (8, 4, 1), (16, 4, 2), (32, 4, 4), (64, 2, 4)]   # (largest D, R, S)


def xlat_form(D):
    R, S = next((R, S) for top, R, S in XLAT_BUCKETS if D <= top)
    a = 0
    while (R * D) % (2 << a) == 0:     # 2^a: the largest power of two in R D
        a += 1
    return R, S, 256 * R // S, a


def xlat_lc(L, S):
    return ceil_div(ceil_div(L, S), 8) * 8


def xlat_lds(D, L):
    R, S, T, a = xlat_form(D)
    wn = T * D + L + 8
    return (wn + (wn >> a) + 1) * 8


def bucket_ends(form, values):
    ends = {}
    for v in values:
        lo, hi = ends.get(form(v), (v, v))
        ends[form(v)] = (min(lo, v), max(hi, v))
    return sorted({v for lo_hi in ends.values() for v in lo_hi})


XLAT_ENDS = bucket_ends(lambda D: xlat_form(D)[:2], range(1, 65))
XLAT_ODD = [3, 7, 63]      # odd D: the smallest LDS shift a of their R (the densest padding), one per R
XLAT_TOPS = [top for top, _, _ in XLAT_BUCKETS]
XLAT_LARGEST = max(((D, 1024) for D in range(1, 65)), key=lambda c: xlat_lds(*c))


def xlat_cases():
    cases = []
    for D in sorted(set(XLAT_ENDS + XLAT_ODD)):
        S = xlat_form(D)[1]
        # 9: part 1 holds one tap, later parts none (S > 1); 8 S + 1: one past a multiple of 8 S
        Ls = {1, 9, 8 * S + 1, 127}
        if D in XLAT_TOPS or (D, 1024) == XLAT_LARGEST:
            Ls |= {1023, 1024}
        cases += [(D, L) for L in sorted(Ls)]
    return cases


# k_resamp<R,P>
def resamp_form(I, D):
    R, P = (8, 1) if D <= I else (8, 0) if D <= 2 * I else (4, 0) if D <= 4 * I else (2, 0) if D <= 8 * I else (1, 0)
    G = max(1, min(256 // I, 8192 // (R * D)))
    return R, P, G, G * R


def resamp_shift(I, D):
    """The a of a padded image (sample s at entry s + (s >> a)): among 31 (none), 6 .. 1 the first with
    the smallest worst number of entries on one bank pair, over the groups of 32 lanes and 64 window
    offsets (nsh_resamp.hip's worst_multiplicity; distinct entries only, so for I = 1 alone)."""
    assert I == 1
    R, P, G, U = resamp_form(I, D)
    if P:
        return 31
    w = np.arange(-(-G // 32) * 32)
    best, shift = 1 << 30, 31
    for a in (31, 6, 5, 4, 3, 2, 1):
        s = np.arange(64)[:, None] + w[None, :] * (R * D)
        bank = ((s + (s >> min(a, 30))) & 31).reshape(64, -1, 32)
        live = (w < G).reshape(1, -1, 32)
        m = int(((bank[..., None] == np.arange(32)) & live[..., None]).sum(axis=2).max())
        if m < best:
            best, shift = m, a
    return shift


def resamp_lds(I, D, L):
    R, P, G, U = resamp_form(I, D)
    Q = ceil_div(L, I)
    a = resamp_shift(I, D)
    wn = U * D + Q - 1
    hs_at = (max(wn + (wn >> a) + 1, U * I) + 1) // 2 * 2
    return hs_at * 8 + Q * I * 4


RESAMP_I = [1, 3, 7, 64]
RESAMP_ODD_TILE = [(1, 37), (3, 37)]
RESAMP_LONG = [(1, 1), (1, 2), (1, 4), (1, 8), (1, 9)]        # one pair per instantiation, Q = 1024 at L = 1024
RESAMP_MOST_INPUTS = max(((1, D) for D in range(33, 65)), key=lambda c: resamp_form(*c)[3] * c[1])


def resamp_pairs():
    pairs = []
    for I in RESAMP_I:
        for D in (1, I, I + 1, 2 * I, 2 * I + 1, 4 * I, 4 * I + 1, 8 * I, 8 * I + 1, 64):
            if 1 <= D <= 64 and (I, D) not in pairs:
                pairs.append((I, D))
    return pairs + RESAMP_ODD_TILE + [(63, 64), (64, 63)]


def resamp_cases(largest=None):
    cases = [(I, D, L) for I, D in resamp_pairs() for L in sorted({max(1, I - 1), I + 1})]
    long_pairs = RESAMP_LONG + [RESAMP_MOST_INPUTS] + ([largest] if largest else [])
    return cases + [(I, D, L) for I, D in dict.fromkeys(long_pairs) for L in (1023, 1024)]


# the I = 1 pair with the largest LDS image at 1024 taps (recomputed and pinned by the CPU test below)
RESAMP_LARGEST = (1, 42)


# k_arb<R,P>: the step is s 2^27, the rate passed 32 F / s, s in [F / 2, 2048 F]
def arb_form(F, L, s):
    Q = ceil_div(L, F)
    step, unit = s << 27, F << 32
    t_fit = ((8192 - Q) * unit - 1) // step + 1
    R, P = (4, 1) if step <= unit else (4, 0) if t_fit >= 1024 else (2, 0) if t_fit >= 512 else (1, 0)
    return R, P, min(R * 256, t_fit) & ~1, t_fit


def arb_boundaries(F, L):
    """The s on both sides of every change of instantiation, the smallest (r = 64) and the largest
    (r = 1/64): step == unit at s = 32 F, and t_fit, which never rises with s, by bisection."""
    s_lo, s_hi = F // 2, 2048 * F
    found = {s_lo, s_hi, 32 * F, 32 * F + 1}
    for t in (1024, 512):
        lo, hi = 32 * F + 1, s_hi           # t_fit(lo) >= t > t_fit(hi)
        assert arb_form(F, L, lo)[3] >= t > arb_form(F, L, hi)[3]
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if arb_form(F, L, mid)[3] >= t else (lo, mid)
        found |= {lo, hi}
    return sorted(found)


ARB_F = [2, 4, 32, 64]


def arb_cases():
    return [(F, L, s) for F in ARB_F for L in sorted({1, F + 1, 2047, 2048}) for s in arb_boundaries(F, L)]


# k_pfb<M>
PFB_M = [2, 4, 8, 16, 32, 64]


def pfb_qmax(M):
    return min(32, 1024 // M)       # at most 32 taps per branch and 1024 taps


def pfb_lds(M, L):
    """The window rows (one free row after every 8 below M = 32), the taps padded to 4 rows, 4 store images."""
    T, Q = 2048 // M, ceil_div(L, M)
    rows = T + Q - 1
    return (rows + (rows >> 3) if M < 32 else rows) * M * 8 + ceil_div(Q, 4) * 4 * M * 4 + 4 * (64 * 4 + 64) * 8


def pfb_cases():
    cases = []
    for M in PFB_M:
        Qm = pfb_qmax(M)
        # Q = 1, 1, 2, 3 (Q mod 4 = 3), 5, and the longest filter with a partial and a full last row
        Ls = {1, M - 1, M + 1, 3 * M - 1, 5 * M, (Qm - 1) * M + 1, Qm * M}
        cases += [(M, L) for L in sorted(Ls)]
    return cases


# ---- the stream forms: data, checks, one guarded call ----------------------------------------------
GUARD = 9 - 9j


def float_taps(rng, L):
    return (rng.choice([-1.0, 1.0], L) * rng.uniform(0.5, 1.0, L)).astype(np.float32)


def make_data(data, L, n_in, H, seed):
    """(taps, samples, the H samples before them) of one data class."""
    rng = np.random.default_rng(seed)
    if data == "int":
        return int_taps(rng, L), int_signal(rng, n_in), int_signal(rng, max(H, 1))[:H]
    return float_taps(rng, L), orc.synth(n_in, 5 + seed), orc.synth(max(H, 1), 10 ** 7 + seed)[:H]


def check(data, what, y, ref):
    """Integer data: bit for bit, the first mismatching index named. Float data: tol_ok."""
    if data == "int":
        y = np.asarray(y, np.complex128).ravel()
        ref = np.asarray(ref, np.complex128).ravel()
        print(what, first_mismatch(y, ref))
        np.testing.assert_array_equal(y, ref, err_msg="%s: %s" % (what, first_mismatch(y, ref)))
    else:
        ok, err, scale = orc.tol_ok(y, ref)
        print(what, "max error", err, "scale", scale)
        assert ok, (what, err, scale)


def check_hist(what, got, raw, end, H):
    """hist_out: the H raw samples before stream sample `end`; raw = [history | samples]."""
    want = raw[end:end + H]
    np.testing.assert_array_equal(got, want, err_msg="%s hist_out: %s" % (what, first_mismatch(got, want)))


def run_call(torch, n_items, H, off, call, aligned=None):
    """One call into an output between guard words, 8 off bytes past a 16-byte boundary; returns
    (the n_items outputs, hist_out). call(out pointer, hist_out tensor) launches."""
    dho = torch.full((max(H, 1),), 5 + 5j, dtype=torch.complex64, device="cuda")
    dy = torch.full((n_items + 8,), GUARD, dtype=torch.complex64, device="cuda")
    o = 2 + off
    p = dy.data_ptr() + 8 * o
    assert dy.data_ptr() % 16 == 0 and p % 16 == 8 * off
    if aligned is not None:
        assert (p % 16 == 0) == aligned
    call(p, dho)
    y = host(dy)
    assert np.all(y[:o] == GUARD) and np.all(y[o + n_items:] == GUARD), "guard words around the output overwritten"
    return y[o:o + n_items].copy(), host(dho)[:H].copy()


def _margin(y, ref):
    err, scale = np.abs(y - ref), np.max(np.abs(ref))
    return float(np.max(err / (1e-5 * np.abs(ref) + 1e-6 * scale)))


def _large_small_large(run, large, small):
    """Both plans exist before the first launch; the large image, the small one, the large one again."""
    for plan in (large, small, large):
        run(plan)
    large[0].close()
    small[0].close()


# ---- positions ----------------------------------------------------------------------------------------
def positions_matrix(D):
    """MFMA and exact forms: the outputs of one 2048-sample chunk."""
    return 2048 // D


def positions_direct(D):
    """k_fir_direct<D,R>: 256 lanes of R outputs."""
    return 256 * DIRECT_R[D]


POSITIONS_ROTATE = 1024
