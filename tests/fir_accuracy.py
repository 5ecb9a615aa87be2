"""What tests/test_gpu_fir_accuracy.py judges the time-domain kernels by: fft_accuracy's two figures
(rms error of the whole call and of its worst position, over the rms of the reference) held to a
small factor of the same figures of an fp32 model that sums in the order the kernel's header documents.

References: the float64 definitions on the same fp32 inputs (xlat_ref, resamp_ref, arb_ref, pfb_ref
here, the synthesizer's polyphase model of tests/test_gpu_pfb_synth.py; fir_ref is xlat_ref untuned).
tests/test_gpu_stream_forms.py takes its references and its fp32 emulation from here.

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

from tests import fft_accuracy as fa
from tests.fft_accuracy import MIN_FRAMES, MIN_OUTPUTS, frames_for, stats  # noqa: F401  (re-exported)

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
def phasors(first, n, inc):
    idx = (np.uint64(first % 2 ** 64) + np.arange(n, dtype=np.uint64))      # wraps mod 2^64
    p = idx * np.uint64(inc)
    turns = (p >> np.uint64(11)).astype(np.float64) / 2.0 ** 53
    return np.exp(2j * np.pi * turns)


def xlat_ref(x, hist, taps, D, inc, first, n_out):
    """y[m] = sum_k h[k] rot(x)[mD - k]; hist = the L-1 raw samples before x[0]."""
    L = len(taps)
    ext = np.concatenate([hist.astype(np.complex128), x.astype(np.complex128)])
    with np.errstate(over="ignore"):
        ext = ext * phasors(first - (L - 1), ext.size, inc)
    return np.convolve(ext, np.asarray(taps, np.float64))[L - 1::D][:n_out]


def xlat_ref_at(x, hist, taps, D, inc, first, n_out):
    """xlat_ref's definition evaluated at the n_out decimated outputs alone, tap by tap in float64 (the
    full-rate convolution of 2^16 D samples with 1024 taps takes a minute at D = 64).
    test_cpu_decimated_reference_is_xlat_ref holds the two together."""
    L = len(taps)
    ext = np.concatenate([hist[:L - 1].astype(np.complex128), x.astype(np.complex128)])
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
    """y[n] = sum_q h[phi + q I] x[j0 - q], phi = (n D) mod I, j0 = floor(n D / I); hist = the Q-1 samples before x[0]."""
    L = len(taps)
    Q = ceil_div(L, I)
    H = Q - 1
    ext = np.concatenate([hist.astype(np.complex128), x[:n_units * D].astype(np.complex128)])
    h = np.zeros(Q * I)
    h[:L] = taps
    n = np.arange(n_units * I)
    j0, phi = n * D // I, n * D % I
    y = np.zeros(n.size, np.complex128)
    for q in range(Q):
        y += h[phi + q * I] * ext[H + j0 - q]
    return y


def arb_indices(step, F, phase, n_out):
    """i, j (int64) and mu (float32, as the kernel forms it) of the outputs 0 .. n_out-1."""
    pos = np.uint64(phase) + np.arange(n_out, dtype=np.uint64) * np.uint64(step)   # below 2^57 here
    k = (pos >> np.uint64(32)).astype(np.int64)
    frac = (pos & np.uint64(0xffffffff)).astype(np.uint32)
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
    ext = np.concatenate([hist.astype(np.complex128), x.astype(np.complex128)])
    h = np.asarray(taps, np.float64)
    d = diff_taps(taps).astype(np.float64)
    mu = mu.astype(np.float64)
    y = np.zeros(n_out, np.complex128)
    for q in range(Q):
        t = j + q * F
        tc = np.minimum(t, L - 1)
        y += np.where(t < L, (h[tc] + mu * d[tc]) * ext[i - q + H], 0)
    return y


def pfb_ref(x, hist, taps, M, n_out):
    """(n_out, M): y[m][c] = sum_p u_p[m] exp(2j pi c p / M), u_p[m] = sum_q h[p + q M] x[(m - q) M - p];
    hist = the L-1 samples before x[0]. Channels 0 and M/2 are the plain and the alternating sum of
    the branches: exact on integer data."""
    L = len(taps)
    Q = ceil_div(L, M)
    ext = np.concatenate([np.zeros(Q * M, np.complex128), hist.astype(np.complex128), x.astype(np.complex128)])
    at0 = Q * M + L - 1                                   # x[0]
    h = np.zeros(Q * M)
    h[:L] = taps
    m, p = np.arange(n_out)[:, None], np.arange(M)[None, :]
    u = np.zeros((n_out, M), np.complex128)
    for q in range(Q):
        u += h[p + q * M] * ext[at0 + (m - q) * M - p]
    c = np.arange(M)
    y = u @ np.exp(2j * np.pi * ((p.T * c[None, :]) % M) / M)
    y[:, 0] = u.sum(axis=1)
    y[:, M // 2] = (u * (1 - 2 * (p % 2))).sum(axis=1)
    return y


def synth_ref(x, hist, taps, M):
    """The synthesizer's float64 polyphase model (tests/test_gpu_pfb_synth.py), on flat arrays."""
    from tests.test_gpu_pfb_synth import ref_of

    return ref_of(x, hist if hist is not None and hist.size else None, taps, M)


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


def xlat_form(D):
    """(R, S) of k_fir_xlat by decimation (nsh_xlat.hip's instantiations)."""
    return next((R, S) for top, R, S in [(4, 8, 1), (8, 4, 1), (16, 4, 2), (32, 4, 4), (64, 2, 4)] if D <= top)


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


# ---- positions ----------------------------------------------------------------------------------------
def positions_matrix(D):
    """MFMA and exact forms: the outputs of one 2048-sample chunk."""
    return 2048 // D


def positions_direct(D):
    """k_fir_direct<D,R>: 256 lanes of R outputs (R: tests/test_gpu_fir_forms.py's DIRECT_R)."""
    from tests.test_gpu_fir_forms import DIRECT_R

    return 256 * DIRECT_R[D]


POSITIONS_ROTATE = 1024
