"""GPU parity of k_pfb_synth<M> (nsh_pfb_synth.hip) at every form, in the manner of
tests/test_gpu_stream_forms.py, whose data classes, guard-word runner and comparisons it uses.

For every M the filters are k_pfb's list: Q = 1 (one tap; M - 1 taps: a branch without one), 2, 3 (a
last chunk of three taps and one padded row), 5 and the longest filter (32 taps per branch, 16 at
M = 64) with a partial and a full last row. Each case runs two chained calls, 2 T + 77 items from a
nonzero history into an output between guard words, 8 bytes off a 16-byte boundary in half of the
cases, then 3 items fed the first call's hist_out.

  * int: outputs r = 0 and r = M/2 of every item are the plain and the alternating sum of the item's
    channels (at most 64 8 per component) through integer taps (at most 32 terms of 8 512): integers
    far below 2^24 whatever the order, so they must equal the float64 reference bit for bit; at M = 2
    every output. The other outputs, whose twiddles are not integers, are judged with tol_ok.
  * float: judged with tol_ok (1e-5) against the float64 polyphase model.

test_synth_forms_fp32_order_stays_inside_the_tolerance (no GPU) emulates in numpy the fp32 q-ascending
branch sum of the longest filter (M = 32, Q = 32) on the float class's data, the DFT in double and
rounded once to fp32, and measures the worst err / (1e-5 |ref| + 1e-6 scale); it asserts at most 0.5.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from newsched_amd import nsh
from tests import fir_accuracy as sf

gpu = pytest.mark.gpu


def branch_inputs(ext, M):
    """v_r[m] = sum_c ext[m][c] exp(2j pi c r / M) in float64; r = 0 and r = M/2 as the plain and the
    alternating sum: exact on integer data."""
    c = np.arange(M)
    v = ext @ np.exp(2j * np.pi * (np.outer(c, c) % M) / M)
    v[:, 0] = ext.sum(axis=1)
    v[:, M // 2] = (ext * (1 - 2 * (c % 2))).sum(axis=1)
    return v


def synth_ref_exact(x, hist, taps, M):
    """(n, M): synth_ref with the DFT written out (branch_inputs); x and hist flat."""
    L = len(taps)
    Q = sf.ceil_div(L, M)
    n = x.size // M
    ext = np.concatenate([hist, x]).astype(np.complex128).reshape(Q - 1 + n, M)
    v = branch_inputs(ext, M)
    hp = np.zeros(Q * M)
    hp[:L] = taps
    y = np.zeros((n, M), np.complex128)
    for q in range(Q):
        y += hp[q * M:(q + 1) * M][None, :] * v[Q - 1 - q:Q - 1 - q + n]
    return y


def synth_cases():
    return sf.pfb_cases()       # the same limits, geometry and tap walk


# ---- CPU -------------------------------------------------------------------------------------------
def test_synth_forms_case_list():
    assert [sf.pfb_qmax(M) for M in sf.PFB_M] == [32, 32, 32, 32, 32, 16]
    cases = synth_cases()
    assert len(cases) == 6 * 7 - 1                        # M = 2: M - 1 and 1 are one filter
    assert [L for M, L in cases if M == 2] == [1, 3, 5, 10, 63, 64]
    assert [L for M, L in cases if M == 16] == [1, 15, 17, 47, 80, 497, 512]
    assert [L for M, L in cases if M == 64] == [1, 63, 65, 191, 320, 961, 1024]
    for M in sf.PFB_M:
        assert sorted({sf.ceil_div(L, M) for m, L in cases if m == M}) == [1, 2, 3, 5, sf.pfb_qmax(M)]
    # the LDS image is k_pfb's: the largest is M = 32's, among the cases
    assert max(sf.pfb_lds(*c) for c in cases) == sf.pfb_lds(32, 1024) == 38656
    for M in sf.PFB_M:       # one tap more than the longest filter is refused before any device call
        with pytest.raises(nsh.NshError, match="at most 32 taps per branch|ntaps must be in"):
            nsh.PfbSynthPlan(np.ones(sf.pfb_qmax(M) * M + 1, np.float32), M)


def test_synth_forms_reference_is_the_definition():
    """The written-out reference against the normative polyphase model and against the definition
    y[n] = sum_c sum_m' X[m'][c] h[n - m' M] exp(2j pi c n / M), at small shapes."""
    rng = np.random.default_rng(11)
    for M, L in ((2, 1), (2, 5), (4, 31), (8, 19), (16, 16), (64, 65)):
        taps = sf.int_taps(rng, L)
        Q, n = sf.ceil_div(L, M), 12
        x, hist = sf.int_signal(rng, n * M), sf.int_signal(rng, max((Q - 1) * M, 1))[:(Q - 1) * M]
        got = synth_ref_exact(x, hist, taps, M)
        want = sf.synth_ref(x, hist, taps, M).reshape(n, M)
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
        ext = np.concatenate([hist, x]).astype(np.complex128).reshape(-1, M)
        idx = np.arange((Q - 1 + n) * M)
        direct = np.zeros(idx.size, np.complex128)
        for c in range(M):
            u = np.zeros(idx.size, np.complex128)
            u[::M] = ext[:, c]
            direct += np.convolve(u, taps.astype(np.float64))[:idx.size] * np.exp(2j * np.pi * ((c * idx) % M) / M)
        direct = direct[(Q - 1) * M:].reshape(n, M)
        assert np.max(np.abs(got - direct)) <= 1e-12 * np.max(np.abs(direct))
        exact = [0, M // 2]
        np.testing.assert_array_equal(got[:, exact], np.round(direct[:, exact].real) + 1j * np.round(direct[:, exact].imag))


def test_synth_forms_fp32_order_stays_inside_the_tolerance():
    M, Q, n = 32, 32, 64
    rng = np.random.default_rng(98)
    h = sf.float_taps(rng, M * Q)
    ext = orc.synth((n + Q - 1) * M, 34).reshape(n + Q - 1, M).astype(np.complex128)
    v = branch_inputs(ext, M)
    v32 = v.astype(np.complex64)                                   # what the kernel's image holds
    # output (m, r): terms q ascending, h[r + q M] v_r[m - q]
    xw = np.stack([v32[Q - 1 - q:Q - 1 - q + n] for q in range(Q)], axis=2).reshape(n * M, Q)
    xd = np.stack([v[Q - 1 - q:Q - 1 - q + n] for q in range(Q)], axis=2).reshape(n * M, Q)
    hw = np.tile(h.reshape(Q, M).T, (n, 1))
    margin = sf._margin(sf._emulate(hw, xw), (xd * hw.astype(np.float64)).sum(axis=1))
    print("worst err / (1e-5 |ref| + 1e-6 scale): %.3f" % margin)
    assert margin <= 0.5


# ---- GPU: two chained calls per case ---------------------------------------------------------------
def synth_chain(torch, plan, data, h, x, hist, n1, n2, off, what):
    M = plan.nchans
    H = (sf.ceil_div(h.size, M) - 1) * M
    ref = synth_ref_exact(x[:(n1 + n2) * M], hist, h, M)
    raw = np.concatenate([hist, x])
    exact = [0, M // 2]
    hin, pos = hist, 0
    for n in (n1, n2):
        dx, dh = sf.dev(torch, x[pos * M:(pos + n) * M]), sf.dev(torch, hin) if H else None
        y, hin = sf.run_call(torch, n * M, H, off, lambda p, dho: plan(dx, dh, dho, p, n))
        y, r = y.reshape(n, M), ref[pos:pos + n]
        name = "%s items %d..%d" % (what, pos, pos + n)
        if data == "int":
            sf.check("int", name + " outputs 0 and M/2", y[:, exact], r[:, exact])
        sf.check("float", name, y, r)
        pos += n
        sf.check_hist(what, hin, raw, pos * M, H)


@gpu
@pytest.mark.parametrize("data", ["int", "float"])
@pytest.mark.parametrize("M,L", synth_cases())
def test_synth_forms(torch_cuda, M, L, data):
    T = 2048 // M
    H = (sf.ceil_div(L, M) - 1) * M
    h, x, hist = sf.make_data(data, L, (2 * T + 80) * M, H, 1000 * L + M + 1)
    plan = nsh.PfbSynthPlan(h, M)
    assert (plan.kernel, plan.tile) == ("k_pfb_synth<%d>" % M, T), (plan.kernel, plan.tile)
    synth_chain(torch_cuda, plan, data, h, x, hist, 2 * T + 77, 3, (M + L) & 1, "%s L=%d" % (plan.kernel, L))
    plan.close()


@gpu
def test_synth_forms_two_plans_of_one_instantiation(torch_cuda):
    """k_pfb_synth<32>: 1024 taps (32 per branch, 38 656 bytes of LDS: the largest image) and one tap."""
    def make(M, L):
        T = 2048 // M
        h, x, hist = sf.make_data("int", L, (2 * T + 80) * M, (sf.ceil_div(L, M) - 1) * M, 77 * L + M + 1)
        plan = nsh.PfbSynthPlan(h, M)
        assert plan.kernel == "k_pfb_synth<32>"
        return plan, h, x, hist, T

    def run(p):
        plan, h, x, hist, T = p
        synth_chain(torch_cuda, plan, "int", h, x, hist, 2 * T + 77, 3, 0, "two plans L=%d" % h.size)

    sf._large_small_large(run, make(32, 1024), make(32, 1))
