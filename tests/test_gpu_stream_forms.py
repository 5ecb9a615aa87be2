"""GPU parity of the four fused stream kernels at every dispatched form.

k_fir_xlat<R,S> (nsh_xlat.hip), k_resamp<R,P> (nsh_resamp.hip), k_arb<R,P> (nsh_arb.hip) and k_pfb<M>
(nsh_pfb.hip) each pick an instantiation, a tile and an LDS image from their parameters at plan
creation. This file restates those rules in Python, derives from them the shapes on both sides of
every boundary (and the shapes at which the tap walk changes path: the wave split of k_fir_xlat, the
partial tap row, the odd tile of k_resamp, the longest sums and the largest LDS images) and runs each
one as two chained calls: 2 tile + 77 outputs from a nonzero history into an output between guard
words, 8 bytes off a 16-byte boundary in half of the cases, then 3 outputs fed the first call's
hist_out. Every case asserts plan.kernel and plan.tile against the restated dispatch.

Two data classes:
  * int: taps are integers in [-8, 8] with nonzero end taps, samples and history Gaussian integers
    with parts in [-8, 8]. Every partial sum is an integer far below 2^24 (at most 1024 8 8 per
    component), so the fp32 result does not depend on the summation order, the tile, the wave split
    or the cut into calls and must equal the float64 reference bit for bit: a dropped, doubled or
    shifted tap or sample is a mismatch at a named index. k_fir_xlat runs at frequency 0 (phasor
    (1, 0), exact). k_arb runs steps and phases that are multiples of 2^27: mu is a multiple of 1/32,
    d = h[k+1] - h[k] an integer, w = fma(mu, d, h) exact with |w| <= 24, and every partial sum a
    multiple of 1/32 below 1024 24 8, inside 24 bits. k_pfb is exact in channels 0 and M/2 (sums and
    one final difference of the branch sums; every channel at M = 2) and judged with tol_ok in the
    others, whose twiddles are not integers.
  * float: orc.synth samples and taps of equal magnitude (a random sign times uniform [0.5, 1]), so
    that the loss or the doubling of any one tap moves an output by about 1 / (3 sqrt(L)) of the
    scale, far above oracle.tol_ok's 1e-5, with which the class is judged against the float64
    references of test_gpu_xlat / _resamp / _arb / _pfb, restated here per output.
    k_fir_xlat runs at frequency -0.37 from first_index = 2^64 - 1000: the index wraps in the call.

test_stream_forms_fp32_order_stays_inside_the_tolerance (no GPU) emulates in numpy the fp32
q-ascending accumulation of the longest sum each kernel can have, on these taps, and measures the
worst err / (1e-5 |ref| + 1e-6 scale) over 2048 outputs: xlat (1024 terms) 0.22, resamp (1024) 0.18,
arb (1024) 0.18, pfb (32 terms, 32 branches) 0.06. It asserts at most 0.5: a correct fp32 kernel in
the plainest order uses less than half of the tolerance, so a failing float case is the kernel's.
That margin is also what tol_ok cannot see into: tests/test_gpu_fir_accuracy.py gates the same kernels'
rms error, whole and per position, against fp32 models in these orders (tests/fir_accuracy.py).

No case here depends on k_fir_xlat's Lc being a multiple of 8: the walk takes the taps at a part's
edges one by one wherever the part starts, so no output depends on it; it is an alignment choice.
"""
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as orc
from newsched_amd import nsh
# the float64 references per output and the fp32 emulation, shared with the accuracy gate; the dispatch
# restated, the data classes and the checks, shared with tests/test_gpu_pfb_synth_forms.py and the CPU
# layout tests
from tests.fir_accuracy import (ARB_F, PFB_M, RESAMP_LARGEST, RESAMP_LONG, RESAMP_MOST_INPUTS, RESAMP_ODD_TILE, XLAT_ENDS,
                                XLAT_LARGEST, XLAT_ODD, _emulate, _fma32, _large_small_large, _margin, arb_boundaries,
                                arb_cases, arb_form, arb_indices, arb_ref, ceil_div, check, check_hist, diff_taps,
                                float_taps, make_data, pfb_cases, pfb_lds, pfb_qmax, pfb_ref, phasors, resamp_cases,
                                resamp_form, resamp_lds, resamp_pairs, resamp_ref, resamp_shift, run_call, xlat_cases,
                                xlat_form, xlat_lc, xlat_lds, xlat_ref)
from tests.gpu_util import dev, int_signal, int_taps

gpu = pytest.mark.gpu


FIRST = 2 ** 64 - 1000     # k_fir_xlat's first_index: the sample index wraps inside call 1
PHASE_INT = (4 << 32) + (5 << 27)       # k_arb's start phases
PHASE_FLOAT = (4 << 32) + 0x89abcdef


# ---- CPU: the derived lists, pinned -------------------------------------------------------------
def test_stream_forms_xlat_case_list():
    assert XLAT_ENDS == [1, 4, 5, 8, 9, 16, 17, 32, 33, 64]
    assert XLAT_ODD == [3, 7, 63]
    assert [xlat_form(D)[:3] for D in XLAT_ENDS] == [(8, 1, 2048), (8, 1, 2048), (4, 1, 1024), (4, 1, 1024), (4, 2, 512),
                                                    (4, 2, 512), (4, 4, 256), (4, 4, 256), (2, 4, 128), (2, 4, 128)]
    assert [xlat_form(D)[3] for D in (3, 7, 63)] == [3, 2, 1]
    assert all(xlat_form(D)[3] >= xlat_form(odd)[3] for odd in XLAT_ODD for D in range(1, 65)
               if xlat_form(D)[0] == xlat_form(odd)[0])
    # the wave split: L = 9 leaves part 1 one tap and the later parts none; 8 S + 1 is one past 8 S
    for S in (2, 4):
        assert xlat_lc(9, S) == 8 and xlat_lc(8 * S + 1, S) == 16 and xlat_lc(8 * S, S) == 8
    assert xlat_lc(1023, 4) == xlat_lc(1024, 4) == 256 and xlat_lc(127, 4) == 32
    assert XLAT_LARGEST == (63, 1024) and xlat_lds(63, 1024) == 109160       # 106.6 KiB
    assert all(xlat_form(D)[2] * D <= 8192 for D in range(1, 65))
    cases = xlat_cases()
    assert len(cases) == 58 and (63, 1024) in cases and (64, 33) in cases and (17, 9) in cases
    assert sorted({L for D, L in cases if D == 32}) == [1, 9, 33, 127, 1023, 1024]


def test_stream_forms_resamp_case_list():
    assert resamp_pairs() == [(1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (1, 8), (1, 9), (1, 64),
                              (3, 1), (3, 3), (3, 4), (3, 6), (3, 7), (3, 12), (3, 13), (3, 24), (3, 25), (3, 64),
                              (7, 1), (7, 7), (7, 8), (7, 14), (7, 15), (7, 28), (7, 29), (7, 56), (7, 57), (7, 64),
                              (64, 1), (64, 64), (1, 37), (3, 37), (63, 64), (64, 63)]
    names = {(I, D): "%d,%d" % resamp_form(I, D)[:2] for I, D in resamp_pairs()}
    assert [names[1, D] for D in (1, 2, 3, 4, 5, 8, 9)] == ["8,1", "8,0", "4,0", "4,0", "2,0", "2,0", "1,0"]
    assert [names[3, D] for D in (3, 4, 6, 7, 12, 13, 24, 25)] == ["8,1", "8,0", "8,0", "4,0", "4,0", "2,0", "2,0", "1,0"]
    assert [names[7, D] for D in (7, 8, 14, 15, 28, 29, 56, 57)] == ["8,1", "8,0", "8,0", "4,0", "4,0", "2,0", "2,0", "1,0"]
    assert sorted({"%d,%d" % resamp_form(I, D)[:2] for I, D in RESAMP_LONG}) == ["1,0", "2,0", "4,0", "8,0", "8,1"]
    # the tile bound 8192 / (R D) binds at I = 1 from D = 33 and can leave an odd number of outputs
    assert resamp_form(1, 32)[2] == 256 and resamp_form(1, 33)[2] == 248
    assert resamp_form(1, 37)[3] * 1 == 221 and resamp_form(3, 37)[3] * 3 == 255 and resamp_form(1, 64)[3] == 128
    assert RESAMP_MOST_INPUTS == (1, 64)
    # the largest image: the a = 1 padding (half as much again) outweighs D = 64's 8192 inputs
    sizes = {D: resamp_lds(1, D, 1024) for D in range(33, 65)}
    assert max(sizes, key=sizes.get) == RESAMP_LARGEST[1] and resamp_shift(1, 42) == 1
    assert sizes[42] == 114656 and sizes[64] == 78976 and max(sizes.values()) <= 112 * 1024
    assert len(resamp_cases(RESAMP_LARGEST)) == 2 * 34 + 2 * 7
    # fewer taps than phases, with phases past L among the outputs (I does not divide D)
    tapless = [(I, D) for I, D, L in resamp_cases() if L < I and D % I]
    assert {(64, 1), (64, 63), (63, 64), (3, 1), (7, 64)} <= set(tapless), tapless


def test_stream_forms_arb_case_list_and_exact_steps():
    """The s on both sides of every boundary, and step_of(32 F / s) = s 2^27 for every s in range."""
    # the boundaries at (32, 384) and (2, 2048) observed at 2^28 granularity: 512 | 513, 4093 | 4094, 8196 | 8197
    # and 32 | 33, 224 | 225, 448 | 449 -- twice those in units of 2^27, refined by one bit
    assert arb_boundaries(32, 384) == [16, 1024, 1025, 8187, 8188, 16392, 16393, 65536]
    assert arb_boundaries(2, 2048) == [1, 64, 65, 448, 449, 897, 898, 4096]
    assert arb_boundaries(2, 1) == [1, 64, 65, 512, 513, 1025, 1026, 4096]
    assert arb_boundaries(64, 2048) == [32, 2048, 2049, 16335, 16336, 32703, 32704, 131072]
    for F, L in ((2, 2048), (4, 5)):     # the bisection against every s
        lo = F // 2
        forms = [arb_form(F, L, s)[:2] for s in range(lo, 2048 * F + 1)]
        edges = [lo + i for i in range(1, len(forms)) if forms[i] != forms[i - 1]]
        assert sorted({lo, 2048 * F} | {s for e in edges for s in (e - 1, e)}) == arb_boundaries(F, L)
        assert sorted(set(forms)) == [(1, 0), (2, 0), (4, 0), (4, 1)]
    for F, L, s in arb_cases():
        R, P, T, t_fit = arb_form(F, L, s)
        assert 110 <= T <= 1024 and T % 2 == 0
    assert arb_form(2, 2048, 64)[:3] == (4, 1, 1024) and arb_form(2, 2048, 65)[:3] == (4, 0, 1024)
    assert [arb_form(32, 384, s)[3] for s in (8187, 8188, 16392, 16393)] == [1024, 1023, 512, 511]
    assert arb_form(2, 2048, 4096)[2:] == (112, 112) and arb_form(2, 1, 4096)[2:] == (128, 128)
    assert len(arb_cases()) == 8 * 4 * 4
    for F in ARB_F:
        for s in range(F // 2, 2048 * F + 1):
            assert nsh.arb_step(32.0 * F / s, F) == s << 27, (F, s)


def test_stream_forms_pfb_case_list():
    assert [pfb_qmax(M) for M in PFB_M] == [32, 32, 32, 32, 32, 16]
    cases = pfb_cases()
    assert [L for M, L in cases if M == 2] == [1, 3, 5, 10, 63, 64]
    assert [L for M, L in cases if M == 32] == [1, 31, 33, 95, 160, 993, 1024]
    assert [L for M, L in cases if M == 64] == [1, 63, 65, 191, 320, 961, 1024]
    assert sorted({ceil_div(L, M) for M, L in cases if M == 16}) == [1, 2, 3, 5, 32]
    # the largest LDS image is k_pfb<32>'s, not k_pfb<64>'s (16 taps per branch); it is among the cases
    assert max(pfb_lds(*c) for c in cases) == pfb_lds(32, 1024) == pfb_lds(32, 993) == 38656
    assert [pfb_lds(M, pfb_qmax(M) * M) for M in PFB_M] == [29472, 30272, 31872, 35072, 38656, 38400]
    assert max(pfb_lds(M, L) for M in PFB_M for L in range(1, pfb_qmax(M) * M + 1)) == 38656
    for M in PFB_M:       # one tap more than the longest filter is refused before any device call
        with pytest.raises(nsh.NshError, match="at most 32 taps per branch|ntaps must be in"):
            nsh.PfbPlan(np.ones(pfb_qmax(M) * M + 1, np.float32), M)


def test_stream_forms_references_are_the_definitions():
    """The per-output references against the definitions the four older GPU files use (zero-stuff and
    convolve; one modulated convolution per channel), at small shapes."""
    rng = np.random.default_rng(7)
    x, hist = int_signal(rng, 600), int_signal(rng, 40)
    for I, D, L in ((3, 2, 17), (1, 5, 9), (7, 3, 5), (4, 4, 1)):
        taps = int_taps(rng, L)
        H = ceil_div(L, I) - 1
        n_units = 30
        ext = np.concatenate([hist[:H], x[:n_units * D]]).astype(np.complex128)
        u = np.zeros(ext.size * I, np.complex128)
        u[::I] = ext
        want = np.convolve(u, taps.astype(np.float64))[H * I::D][:n_units * I]
        np.testing.assert_array_equal(resamp_ref(x, hist[:H], taps, I, D, n_units), want)
    for M, L in ((2, 5), (8, 19), (4, 3), (16, 16)):
        taps = int_taps(rng, L)
        n_out = 20
        ext = np.concatenate([hist[:L - 1], x[:n_out * M]]).astype(np.complex128)
        k = np.arange(L)
        got = pfb_ref(x[:n_out * M], hist[:L - 1], taps, M, n_out)
        for c in range(M):
            want = np.convolve(ext, taps * np.exp(2j * np.pi * ((c * k) % M) / M))[L - 1::M][:n_out]
            assert np.max(np.abs(got[:, c] - want)) <= 1e-12 * np.max(np.abs(want))
            if c in (0, M // 2):
                np.testing.assert_array_equal(got[:, c], np.round(want.real) + 1j * np.round(want.imag))
    F, L, step, phase = 4, 11, 37 << 27, PHASE_INT        # arb: each output from its own window, tap by tap
    taps = int_taps(rng, L)
    H = ceil_div(L, F) - 1
    got = arb_ref(x, hist[:H], taps, F, step, phase, 50)
    d = diff_taps(taps)
    raw = np.concatenate([hist[:H], x]).astype(np.complex128)
    for n in range(50):
        pos = phase + n * step
        i, j, mu = (pos >> 32) // F, (pos >> 32) % F, float(np.float32((pos & 0xffffffff) >> 8) * np.float32(2.0 ** -24))
        want = sum((float(taps[t]) + mu * float(d[t])) * raw[H + i - q] for q in range(H + 1) for t in [j + q * F] if t < L)
        assert got[n] == want, (n, got[n], want)


def test_stream_forms_fp32_order_stays_inside_the_tolerance():
    """An fp32 emulation of the q-ascending sum, at the longest sum of each kernel and on the float
    class's taps and samples, uses at most half of tol_ok's per-element bound (the norm-wise bound,
    1e-5 scale, is ten times the smallest per-element one)."""
    n = 2048
    rng = np.random.default_rng(99)
    win = np.lib.stride_tricks.sliding_window_view
    margins = {}
    # xlat, L = 1024, D = 1: the samples rotated once (rounded to fp32), reversed taps q ascending
    h = float_taps(rng, 1024)
    x = orc.synth(n + 1023, 31)
    inc = int(round(0.37 * 2 ** 64))
    rot = x.astype(np.complex128) * phasors(FIRST, x.size, inc)
    xw = win(rot.astype(np.complex64), 1024)
    g = np.broadcast_to(h[::-1], xw.shape)
    margins["xlat"] = _margin(_emulate(g, xw), (win(rot, 1024) * h[::-1].astype(np.float64)).sum(axis=1))
    # resamp, I = D = 1, L = 1024: tap q meets x[j0 - q]
    xw = win(x, 1024)[:, ::-1]
    margins["resamp"] = _margin(_emulate(np.broadcast_to(h, xw.shape), xw),
                                (xw.astype(np.complex128) * h.astype(np.float64)).sum(axis=1))
    # arb, F = 2, L = 2048, Q = 1024 at r = 1 / 1.37: w = fl32(mu d + h)
    F, L, step, phase = 2, 2048, int(1.37 * (2 << 32)), PHASE_FLOAT
    h2 = float_taps(rng, L)
    d2 = diff_taps(h2)
    i, j, mu = arb_indices(step, F, phase, n)
    xs = orc.synth(int(i.max()) + 1 + 1023, 32)
    t = j[:, None] + np.arange(1024)[None, :] * F
    xw = xs[1023 + i[:, None] - np.arange(1024)[None, :]]
    w = _fma32(np.broadcast_to(mu[:, None], t.shape), d2[t], h2[t])
    ref = ((h2[t].astype(np.float64) + mu[:, None].astype(np.float64) * d2[t]) * xw).sum(axis=1)
    margins["arb"] = _margin(_emulate(w, xw), ref)
    # pfb, M = 32, L = 1024: 32 branch sums of 32 terms in fp32, the DFT across them in double
    M, Q = 32, 32
    h3 = float_taps(rng, M * Q)
    steps = n // M
    xp = orc.synth((steps + Q) * M, 33).reshape(steps + Q, M)[:, ::-1]      # [time step][branch p]
    xw = np.stack([xp[Q - q: Q - q + steps] for q in range(Q)], axis=2).reshape(steps * M, Q)
    hw = np.tile(h3.reshape(Q, M).T, (steps, 1))
    E = np.exp(2j * np.pi * np.outer(np.arange(M), np.arange(M)) / M)
    ref = (xw.astype(np.complex128) * hw).sum(axis=1).reshape(steps, M) @ E
    margins["pfb"] = _margin(_emulate(hw, xw).reshape(steps, M) @ E, ref)
    print("worst err / (1e-5 |ref| + 1e-6 scale):", {k: round(v, 3) for k, v in margins.items()})
    assert all(v <= 0.5 for v in margins.values()), margins


# ---- GPU: two chained calls per case -------------------------------------------------------------------
def xlat_chain(torch, plan, data, h, x, hist, first, n1, n2, off, what):
    D, H = plan.decim, h.size - 1
    ref = xlat_ref(x, hist, h, D, plan.inc, first, n1 + n2)
    raw = np.concatenate([hist, x])
    hin, pos = hist, 0
    for n in (n1, n2):
        dx, dh = dev(torch, x[pos * D:(pos + n) * D]), dev(torch, hin) if H else None
        y, hin = run_call(torch, n, H, off, lambda p, dho: plan(dx, dh, dho, p, n, first + pos * D))
        check(data, "%s outputs %d..%d" % (what, pos, pos + n), y, ref[pos:pos + n])
        pos += n
        check_hist(what, hin, raw, pos * D, H)


@gpu
@pytest.mark.parametrize("data", ["int", "float"])
@pytest.mark.parametrize("D,L", xlat_cases())
def test_stream_forms_xlat(torch_cuda, D, L, data):
    """k_fir_xlat<R,S> at both ends of every D bucket and at the odd D of the smallest LDS shift, with
    1, 9, 8 S + 1 and 127 taps (1023 and 1024 at the buckets' upper ends and at D = 63, the largest
    LDS image)."""
    R, S, T, a = xlat_form(D)
    h, x, hist = make_data(data, L, (2 * T + 80) * D, L - 1, 1000 * L + D)
    plan = nsh.FirXlatPlan(h, D, 0.0 if data == "int" else -0.37)
    assert (plan.kernel, plan.tile) == ("k_fir_xlat<%d,%d>" % (R, S), T), (plan.kernel, plan.tile)
    # the increment of -freq_norm, from exact rational arithmetic: round(0.37 2^64) of the double 0.37
    assert plan.inc == (0 if data == "int" else round(Fraction(0.37) * 2 ** 64))
    xlat_chain(torch_cuda, plan, data, h, x, hist, FIRST, 2 * T + 77, 3, (D + L) & 1, "%s D=%d L=%d" % (plan.kernel, D, L))
    plan.close()


def resamp_chain(torch, plan, data, h, x, hist, n1, n2, off, what, aligned=None):
    I, D, H = plan.interp, plan.decim, plan.history
    L = h.size
    ref = resamp_ref(x, hist, h, I, D, n1 + n2)
    raw = np.concatenate([hist, x])
    hin, pos = hist, 0
    for n in (n1, n2):
        dx, dh = dev(torch, x[pos * D:(pos + n) * D]), dev(torch, hin) if H else None
        y, hin = run_call(torch, n * I, H, off, lambda p, dho: plan(dx, dh, dho, p, n), aligned)
        check(data, "%s units %d..%d" % (what, pos, pos + n), y, ref[pos * I:(pos + n) * I])
        if L < I:  # phases without a tap (none where I divides D: every output has phase 0)
            phi = np.arange(n * I) * D % I
            assert (phi >= L).any() == (D % I != 0) and np.all(y[phi >= L] == 0), what
        pos += n
        check_hist(what, hin, raw, pos * D, H)


@gpu
@pytest.mark.parametrize("data", ["int", "float"])
@pytest.mark.parametrize("I,D,L", resamp_cases(RESAMP_LARGEST))
def test_stream_forms_resamp(torch_cuda, I, D, L, data):
    """k_resamp<R,P> on both sides of D = I, 2 I, 4 I, 8 I at I = 1, 3, 7, 64, the odd tiles of (1, 37)
    and (3, 37) on a 16-byte aligned output (the 8-byte store path), with max(1, I - 1) and I + 1 taps
    (fewer taps than phases: the outputs of the phases past L are exact zeros); 1023 and 1024 taps
    at one pair per instantiation, at the most inputs per tile and at the largest LDS image."""
    R, P, G, U = resamp_form(I, D)
    H = ceil_div(L, I) - 1
    h, x, hist = make_data(data, L, (2 * U + 80) * D, H, 1000 * L + 64 * I + D)
    plan = nsh.ResampPlan(h, I, D)
    assert (plan.kernel, plan.tile, plan.history) == ("k_resamp<%d,%d>" % (R, P), U, H), (plan.kernel, plan.tile)
    odd = (I, D) in RESAMP_ODD_TILE
    assert not odd or (U * I) % 2 == 1
    off = 0 if odd else (I + D + L) & 1
    resamp_chain(torch_cuda, plan, data, h, x, hist, 2 * U + 77, 3, off, "%s I=%d D=%d L=%d" % (plan.kernel, I, D, L),
                 aligned=True if odd else None)
    plan.close()


def arb_inputs(step, F, phase, n_out):
    """The fewest inputs that hold n_out outputs from phase: i(n_out - 1) + 1."""
    return (((phase + (n_out - 1) * step) >> 32) // F) + 1


def arb_chain(torch, plan, data, h, x, hist, phase, n1, n2, off, what):
    F, H, step = plan.nfilt, plan.history, plan.step
    ref = arb_ref(x, hist, h, F, step, phase, n1 + n2)
    raw = np.concatenate([hist, x])
    hin, at, done = hist, 0, 0
    for n in (n1, n2):
        n_in = arb_inputs(step, F, phase, n)
        n_out, c, nxt = plan.span(phase, n_in, n)
        assert n_out == n and at + n_in <= x.size
        dx, dh = dev(torch, x[at:at + n_in]), dev(torch, hin) if H else None
        y, hin = run_call(torch, n, H, off, lambda p, dho: plan(dx, n_in, dh, dho, p, n, phase))
        check(data, "%s outputs %d..%d" % (what, done, done + n), y, ref[done:done + n])
        at, done, phase = at + c, done + n, nxt
        check_hist(what, hin, raw, at, H)


@gpu
@pytest.mark.parametrize("data", ["int", "float"])
@pytest.mark.parametrize("F,L,s", arb_cases())
def test_stream_forms_arb(torch_cuda, F, L, s, data):
    """k_arb<R,P> at r = 64, r = 1 and the first step above it, on both sides of t_fit = 1024 and
    t_fit = 512 and at r = 1/64 (a tile below the block size), for F = 2, 4, 32, 64 and 1, F + 1, 2047
    and 2048 taps (1024 taps per output at F = 2, a padded tap image at F = 64). The second call
    continues at n_consumed with span's phase_next."""
    R, P, T, t_fit = arb_form(F, L, s)
    H = ceil_div(L, F) - 1
    phase = PHASE_INT if data == "int" else PHASE_FLOAT
    n1, n2 = 2 * T + 77, 3
    n_in = arb_inputs(s << 27, F, phase, n1 + n2) + 2
    h, x, hist = make_data(data, L, n_in, H, 1000 * L + 7 * F + s)
    plan = nsh.ArbPlan(h, 32.0 * F / s, F)
    assert plan.step == s << 27, (plan.step, s)
    assert (plan.kernel, plan.tile, plan.history) == ("k_arb<%d,%d>" % (R, P), T, H), (plan.kernel, plan.tile)
    arb_chain(torch_cuda, plan, data, h, x, hist, phase, n1, n2, (F + L + s) & 1, "%s F=%d L=%d s=%d" % (plan.kernel, F, L, s))
    plan.close()


def pfb_chain(torch, plan, data, h, x, hist, n1, n2, off, what):
    M, H = plan.nchans, h.size - 1
    ref = pfb_ref(x, hist, h, M, n1 + n2)
    raw = np.concatenate([hist, x])
    exact = [0, M // 2]
    hin, pos = hist, 0
    for n in (n1, n2):
        dx, dh = dev(torch, x[pos * M:(pos + n) * M]), dev(torch, hin) if H else None
        y, hin = run_call(torch, n * M, H, off, lambda p, dho: plan(dx, dh, dho, p, n))
        y, r = y.reshape(n, M), ref[pos:pos + n]
        name = "%s steps %d..%d" % (what, pos, pos + n)
        if data == "int":
            check("int", name + " channels 0 and M/2", y[:, exact], r[:, exact])
        check("float", name, y, r)
        pos += n
        check_hist(what, hin, raw, pos * M, H)


@gpu
@pytest.mark.parametrize("data", ["int", "float"])
@pytest.mark.parametrize("M,L", pfb_cases())
def test_stream_forms_pfb(torch_cuda, M, L, data):
    """k_pfb<M> at Q = 1 (one tap; M - 1 taps: a branch without one), 2, 3 (a last chunk of three taps
    and one padded row), 5 and the longest filter (32 taps per branch, 16 at M = 64) with a partial
    and a full last row."""
    T = 2048 // M
    h, x, hist = make_data(data, L, (2 * T + 80) * M, L - 1, 1000 * L + M)
    plan = nsh.PfbPlan(h, M)
    assert (plan.kernel, plan.tile) == ("k_pfb<%d>" % M, T), (plan.kernel, plan.tile)
    pfb_chain(torch_cuda, plan, data, h, x, hist, 2 * T + 77, 3, (M + L) & 1, "%s L=%d" % (plan.kernel, L))
    plan.close()


@gpu
def test_stream_forms_xlat_two_plans_of_one_instantiation(torch_cuda):
    """k_fir_xlat<2,4>: D = 63 with 1024 taps (109 160 bytes of LDS) and the D with the smallest image at one tap."""
    def make(D, L):
        T = xlat_form(D)[2]
        h, x, hist = make_data("int", L, (2 * T + 80) * D, L - 1, 77 * L + D)
        plan = nsh.FirXlatPlan(h, D, 0.0)
        assert plan.kernel == "k_fir_xlat<2,4>"
        return plan, h, x, hist, T

    def run(p):
        plan, h, x, hist, T = p
        xlat_chain(torch_cuda, plan, "int", h, x, hist, FIRST, 2 * T + 77, 3, 0, "two plans D=%d L=%d" % (plan.decim, h.size))

    small = min(range(33, 65), key=lambda D: xlat_lds(D, 1))
    assert 2 * xlat_lds(small, 1) < xlat_lds(63, 1024)
    _large_small_large(run, make(63, 1024), make(small, 1))


@gpu
def test_stream_forms_resamp_two_plans_of_one_instantiation(torch_cuda):
    """k_resamp<1,0>: (1, 42) with 1024 taps (114 656 bytes of LDS, the largest image) and (3, 64) with 2 taps."""
    def make(I, D, L):
        U, H = resamp_form(I, D)[3], ceil_div(L, I) - 1
        h, x, hist = make_data("int", L, (2 * U + 80) * D, H, 77 * L + D)
        plan = nsh.ResampPlan(h, I, D)
        assert plan.kernel == "k_resamp<1,0>"
        return plan, h, x, hist, U

    def run(p):
        plan, h, x, hist, U = p
        resamp_chain(torch_cuda, plan, "int", h, x, hist, 2 * U + 77, 3, 0,
                     "two plans I=%d D=%d L=%d" % (plan.interp, plan.decim, h.size))

    _large_small_large(run, make(*RESAMP_LARGEST, 1024), make(3, 64, 2))


@gpu
@pytest.mark.parametrize("large,small", [((2, 2048, 64), (2, 1, 1)), ((64, 2048, 131072), (2, 1, 4096))],
                         ids=["k_arb<4,1>", "k_arb<1,0>"])
def test_stream_forms_arb_two_plans_of_one_instantiation(torch_cuda, large, small):
    """k_arb<4,1>: F = 2 with 2048 taps at r = 1 (2048 window samples and 2048 tap pairs) and one tap at
    r = 64 (17 window samples). k_arb<1,0>: F = 64 with 2048 taps and F = 2 with one tap at r = 1/64."""
    def make(F, L, s):
        T, H = arb_form(F, L, s)[2], ceil_div(L, F) - 1
        n_in = arb_inputs(s << 27, F, PHASE_INT, 2 * T + 80) + 2
        h, x, hist = make_data("int", L, n_in, H, 77 * L + s)
        plan = nsh.ArbPlan(h, 32.0 * F / s, F)
        assert plan.kernel == "k_arb<%d,%d>" % arb_form(*large)[:2] and plan.step == s << 27
        return plan, h, x, hist, T

    def run(p):
        plan, h, x, hist, T = p
        arb_chain(torch_cuda, plan, "int", h, x, hist, PHASE_INT, 2 * T + 77, 3, 0,
                  "two plans F=%d L=%d step=%d" % (plan.nfilt, h.size, plan.step))

    _large_small_large(run, make(*large), make(*small))


@gpu
def test_stream_forms_pfb_two_plans_of_one_instantiation(torch_cuda):
    """k_pfb<32>: 1024 taps (32 per branch, 38 656 bytes of LDS: the largest image of k_pfb) and one tap."""
    def make(M, L):
        T = 2048 // M
        h, x, hist = make_data("int", L, (2 * T + 80) * M, L - 1, 77 * L + M)
        plan = nsh.PfbPlan(h, M)
        assert plan.kernel == "k_pfb<32>"
        return plan, h, x, hist, T

    def run(p):
        plan, h, x, hist, T = p
        pfb_chain(torch_cuda, plan, "int", h, x, hist, 2 * T + 77, 3, 0, "two plans L=%d" % h.size)

    _large_small_large(run, make(32, 1024), make(32, 1))
