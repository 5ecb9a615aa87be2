"""GPU parity of the base FIR family at every dispatched kernel form.

nsh_fir_plan_create sends a filter to a kernel templated on a tap-count bucket (k_fir_mfma12<Q>,
k_fir_mfma11 / k_fir_mfma13 / k_fir_exact13<D,QH>, k_fir_f32mfma<QF>) or to the direct form
(k_fir_direct<D,R>, every filter the others refuse, up to 4096 taps). This file restates the
bucket formulas, derives both end points of every bucket from them and runs each one; and it
runs the direct form up to 4096 taps at decimations 1, 2, 4 and 8.

Two data classes:
  * integer: taps, samples and history are integers in [-8, 8]. Every partial sum is an integer
    far below 2^24 (about 6000 at 4096 taps), so fp32 accumulation in any order is exact; the
    fp16x2 split scales by powers of two, where a 4-bit integer is exact in the high term and
    has a zero low term. Every form here therefore equals the double-precision oracle bit for
    bit, and a dropped, duplicated or shifted tap or sample is a mismatch at a named index.
  * float: orc.synth samples under oracle.tol_ok (1e-5), which exercises the split's low terms.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from newsched_amd import nsh
from tests.fir_accuracy import AUTO_DIRECT, DIRECT_R, ENDS_12, ENDS_D, ENDS_F32, direct_name, q12, qf
from tests.fir_accuracy import decim_qh as qh
from tests.gpu_util import dev, first_mismatch, host, int_signal, int_taps

pytestmark = pytest.mark.gpu


def run_fir(torch, plan, x, n_out, hist=None, null_hist=False):
    L = plan.ntaps
    dx = dev(torch, x)
    hin = dev(torch, hist if hist is not None else np.zeros(max(L - 1, 1), np.complex64))
    hout = torch.zeros(max(L - 1, 1), dtype=torch.complex64, device="cuda")
    dy = torch.empty(max(n_out, 1), dtype=torch.complex64, device="cuda")
    plan(dx, 0 if null_hist else hin, hout, dy, n_out)
    return host(dy)[:n_out], host(hout)[: L - 1]


def form_cases():
    """(kernel name, decim, L, algo, NSH_DEC_WALK_MASK or None) for both ends of every bucket."""
    cases = [("k_fir_mfma12<%d>" % q12(L), 1, L, nsh.FIR_MFMA, None) for L in ENDS_12]
    for D in (2, 4):
        for kern, mask in (("k_fir_mfma11", "0"), ("k_fir_mfma13", "20")):
            cases += [("%s<%d,%d>" % (kern, D, qh(L, D)), D, L, nsh.FIR_MFMA, mask) for L in ENDS_D[D]]
    cases += [("k_fir_f32mfma<%d>" % qf(L), 1, L, nsh.FIR_MFMA_F32, None) for L in ENDS_F32]
    cases += [(direct_name(D), D, L, nsh.FIR_AUTO, None) for D, L in AUTO_DIRECT.items()]
    return [pytest.param(*c, id="%s-L%d" % (c[0], c[2])) for c in cases]


def test_fir_forms_bucket_end_points():
    """The end points derived from the formulas are the ones the dispatch documents."""
    assert ENDS_12 == [1, 2, 33, 34, 65, 66, 97, 98, 129, 130, 161]
    assert ENDS_D[2] == [1, 32, 33, 64, 65, 96, 97, 128, 129, 160]
    assert ENDS_D[4] == [1, 64, 65, 128, 129, 192, 193, 256, 257, 320]
    assert ENDS_F32 == [1] + [L for q in range(2, 18) for L in (16 * q - 30, 16 * q - 15)]
    assert (len(ENDS_12), len(ENDS_D[2]), len(ENDS_D[4]), len(ENDS_F32)) == (11, 10, 10, 33)
    assert AUTO_DIRECT == {1: 162, 2: 161, 4: 321}


def make_data(data, L, n_in, seed):
    """(taps, samples, history) of one data class."""
    rng = np.random.default_rng(seed)
    if data == "int":
        return int_taps(rng, L), int_signal(rng, n_in), int_signal(rng, max(L - 1, 1))[: L - 1]
    h = (rng.standard_normal(L) * 0.1).astype(np.float32)
    return h, orc.synth(n_in, 5 + seed), orc.synth(max(L - 1, 1), 10 ** 7 + seed)[: L - 1]


def check(data, what, y, ref):
    """Integer data: bit for bit, the first mismatching index named. Float data: tol_ok."""
    if data == "int":
        print(what, first_mismatch(y, ref))
        np.testing.assert_array_equal(y, ref, err_msg="%s: %s" % (what, first_mismatch(y, ref)))
    else:
        ok, err, scale = orc.tol_ok(y, ref)
        print(what, "max error", err, "scale", scale)
        assert ok, (what, err, scale)


def chained_calls(torch, plan, data, h, x, hist, D, n1, n2, what):
    """Two calls on one stream, the second fed the first's hist_out; outputs and both histories
    against the oracle (histories always exactly)."""
    L = h.size
    x1, x2 = x[: n1 * D], x[n1 * D:(n1 + n2) * D]
    y1, h1 = run_fir(torch, plan, x1, n1, hist=hist if L > 1 else None)
    r1, g1 = orc.fir_ccf(x1, h, D, hist=hist if L > 1 else None, return_hist=True)
    check(data, what + " call 1", y1, r1)
    np.testing.assert_array_equal(h1, g1, err_msg=what + " hist_out 1: " + first_mismatch(h1, g1))
    y2, h2 = run_fir(torch, plan, x2, n2, hist=h1 if L > 1 else None)
    r2, g2 = orc.fir_ccf(x2, h, D, hist=g1 if L > 1 else None, return_hist=True)
    check(data, what + " call 2", y2, r2)
    np.testing.assert_array_equal(h2, g2, err_msg=what + " hist_out 2: " + first_mismatch(h2, g2))


# ---- A. every instantiation, at both ends of its bucket -----------------------------------------
@pytest.mark.parametrize("data", ["int", "float"])
@pytest.mark.parametrize("kernel,D,L,algo,mask", form_cases())
def test_fir_forms_every_bucket(torch_cuda, monkeypatch, kernel, D, L, algo, mask, data):
    """Both ends of every tap-count bucket of every matrix form (and the first direct-form tap count
    past each): the plan names exactly the expected kernel, AUTO resolves to the same one where the
    form is AUTO's choice, and two chained calls -- 2 (2048 / D) + 77 outputs with a nonzero history,
    then 3 outputs (shorter than most filters) fed the first call's hist_out -- match the oracle."""
    torch = torch_cuda
    if mask is not None:
        monkeypatch.setenv("NSH_DEC_WALK_MASK", mask)
    n1, n2 = 2 * (2048 // D) + 77, 3
    h, x, hist = make_data(data, L, (n1 + n2) * D, 1000 * L + D)
    plan = nsh.FirPlan(h, D, algo)
    assert plan.kernel == kernel, plan.kernel
    if algo == nsh.FIR_MFMA:  # the exact-fp32 form is never AUTO's choice
        auto = nsh.FirPlan(h, D, nsh.FIR_AUTO)
        assert auto.kernel == kernel, (auto.kernel, kernel)
        auto.close()
    chained_calls(torch, plan, data, h, x, hist, D, n1, n2, "%s L=%d" % (kernel, L))
    plan.close()


def test_fir_forms_auto_switches_to_direct():
    """The last tap count of each matrix form and the first one past it."""
    for D, L in AUTO_DIRECT.items():
        h = np.ones(L, np.float32)
        last = nsh.FirPlan(h[:-1], D, nsh.FIR_AUTO)
        assert last.algo == nsh.FIR_MFMA and last.kernel.startswith("k_fir_mfma1"), (D, L - 1, last.kernel)
        past = nsh.FirPlan(h, D, nsh.FIR_AUTO)
        assert past.algo == nsh.FIR_DIRECT and past.kernel == direct_name(D), (D, L, past.kernel)
        with pytest.raises(nsh.NshError):
            nsh.FirPlan(h, D, nsh.FIR_MFMA)
    with pytest.raises(nsh.NshError):
        nsh.FirPlan(np.ones(ENDS_F32[-1] + 1, np.float32), 1, nsh.FIR_MFMA_F32)


def _nonfinite_pattern(y, ref):
    for f in (np.isnan, np.isinf):
        for part in (np.real, np.imag):
            bad = np.nonzero(f(part(y)) != f(part(ref)))[0]
            assert bad.size == 0, (f.__name__, part.__name__, bad.size, bad[:8].tolist(), bad[-8:].tolist(),
                                   y[bad[:4]].tolist(), ref[bad[:4]].tolist())
    for part in (np.real, np.imag):
        inf = np.isinf(part(y))
        np.testing.assert_array_equal(np.sign(part(y)[inf]), np.sign(part(ref)[inf]))


# one tap count inside each bucket that no test had launched; at decim 1 one whose exact-fp32 tile
# has the blocking of k_fir_f32mfma (QF = 2Q - 1), so the two can be compared bit for bit
EXACT_CASES = [("k_fir_exact12<4>", 1, 90, None), ("k_fir_exact13<2,4>", 2, 81, "20"), ("k_fir_mfma11<2,4>", 2, 81, "0"),
               ("k_fir_exact13<4,5>", 4, 225, "20"), ("k_fir_mfma11<4,5>", 4, 225, "0"),
               ("k_fir_exact13<4,6>", 4, 301, "20"), ("k_fir_mfma11<4,6>", 4, 301, "0")]


@pytest.mark.parametrize("kernel,D,L,mask", [pytest.param(*c, id="%s-L%d" % (c[0], c[2])) for c in EXACT_CASES])
def test_fir_forms_exact_chunks(torch_cuda, monkeypatch, kernel, D, L, mask):
    """The exact-chunk kernels of the buckets above (k_fir_exact12<Q>, k_fir_exact13<D,QH>, and
    k_fir_mfma11's inline exact path): one 2048-input chunk holds a finite 2^40 spike (beyond the
    split's range: the exact-fp32 tile), another a NaN (the fp32 direct form inside the launch).
    As test_fir_mfma_exact_paths: hist_out is bit-identical to k_fir_direct's; the NaN positions
    are k_fir_direct's and the oracle's and the NaN chunk's finite outputs are bit-identical to
    k_fir_direct; at decim 1 the spike chunk is bit-identical to k_fir_f32mfma<2Q-1>; and every
    chunk's finite outputs meet the tolerance on that chunk's own scale."""
    torch = torch_cuda
    if mask is not None:
        monkeypatch.setenv("NSH_DEC_WALK_MASK", mask)
    h = (np.hamming(L) / (L / 2)).astype(np.float32)
    n = 9 * 2048 + 333
    n_out = n // D
    spike, nan = 2, 6  # chunks
    x = orc.synth(n, 5)[: n_out * D]
    x[spike * 2048 + 100] *= np.float32(2.0 ** 40)
    x[nan * 2048 + 100] = complex(np.nan, 0.5)
    plan = nsh.FirPlan(h, D, nsh.FIR_MFMA)
    want = {"k_fir_exact12": "k_fir_mfma12", "k_fir_exact13": "k_fir_mfma13"}
    head, args = kernel.split("<")
    assert plan.kernel == want.get(head, head) + "<" + args, plan.kernel
    y, hy = run_fir(torch, plan, x, n_out)
    yd, hd = run_fir(torch, nsh.FirPlan(h, D, nsh.FIR_DIRECT), x, n_out)
    np.testing.assert_array_equal(hy.view(np.uint32), hd.view(np.uint32))
    ref = orc.fir_ccf(x, h, D)
    _nonfinite_pattern(y, ref)
    _nonfinite_pattern(yd, ref)
    c = 2048 // D
    bad = np.isnan(ref.real) | np.isnan(ref.imag)
    assert bad[nan * c:(nan + 1) * c].any() and not bad[: nan * c].any()
    a, b = nan * c, (nan + 1) * c
    m = ~bad[a:b]
    np.testing.assert_array_equal(y[a:b][m].view(np.uint32), yd[a:b][m].view(np.uint32))
    if D == 1:
        pf = nsh.FirPlan(h, 1, nsh.FIR_MFMA_F32)
        assert pf.kernel == "k_fir_f32mfma<%d>" % (2 * q12(L) - 1), pf.kernel
        yf, _ = run_fir(torch, pf, x, n_out)
        a, b = spike * c, (spike + 1) * c
        np.testing.assert_array_equal(y[a:b].view(np.uint32), yf[a:b].view(np.uint32))
    for a in range(0, n_out, c):  # each chunk on its own scale
        m = ~bad[a:a + c]
        ok, err, scale = orc.tol_ok(y[a:a + c][m], ref[a:a + c][m])
        assert ok, (kernel, a, err, scale)


# ---- B. the direct form up to 4096 taps -----------------------------------------------------------
DIRECT_TAPS = [162, 1000, 2047, 3616, 3617, 4089, 4096]  # odd, L % 8 != 0, both sides of 64 KiB of LDS
DIRECT_T = {D: 256 * R for D, R in DIRECT_R.items()}     # outputs per workgroup


def _firwin(L):
    return np.asarray(__import__("scipy.signal", fromlist=["firwin"]).firwin(L, 0.25), np.float32)


@pytest.mark.parametrize("data", ["int", "float"])
@pytest.mark.parametrize("L", DIRECT_TAPS)
@pytest.mark.parametrize("D", [1, 2, 4, 8])
def test_fir_forms_direct_long(torch_cuda, D, L, data):
    """k_fir_direct<D,R> at 162 .. 4096 taps, at 1, T - 1, T + 1 and 2 T + 3 outputs (T outputs per
    workgroup): its LDS window of (T - 1) D + Lp samples (above 64 KiB from 3617 taps at decim 2, 4
    and 8), the last tap block's rule at L % 8 != 0, and a hist_out that comes from hist_in over
    thousands of samples. Each size is two chained calls (then 3 outputs) from a nonzero history;
    one more call passes hist_in = NULL and must equal the same call on explicit zeros."""
    torch = torch_cuda
    T = DIRECT_T[D]
    assert (T, direct_name(D)) == {1: (2048, "k_fir_direct<1,8>"), 2: (2048, "k_fir_direct<2,8>"),
                                  4: (1024, "k_fir_direct<4,4>"), 8: (512, "k_fir_direct<8,2>")}[D]
    n2 = 3
    h = _firwin(L) if data == "float" else int_taps(np.random.default_rng(100 * L + D), L)
    plan = nsh.FirPlan(h, D, nsh.FIR_DIRECT)
    assert plan.algo == nsh.FIR_DIRECT and plan.kernel == direct_name(D), plan.kernel
    for n1 in (1, T - 1, T + 1, 2 * T + 3):
        _, x, hist = make_data(data, L, (n1 + n2) * D, 100 * L + 10 * D + n1 % 7)
        chained_calls(torch, plan, data, h, x, hist, D, n1, n2, "%s L=%d n_out=%d" % (plan.kernel, L, n1))
    n0 = T + 1
    x0 = x[: n0 * D]
    y0, h0 = run_fir(torch, plan, x0, n0, null_hist=True)
    yz, hz = run_fir(torch, plan, x0, n0, hist=np.zeros(L - 1, np.complex64))
    np.testing.assert_array_equal(y0.view(np.uint32), yz.view(np.uint32))
    np.testing.assert_array_equal(h0.view(np.uint32), hz.view(np.uint32))
    r0, g0 = orc.fir_ccf(x0, h, D, return_hist=True)
    check(data, "%s L=%d null history" % (plan.kernel, L), y0, r0)
    np.testing.assert_array_equal(h0, g0)
    plan.close()


@pytest.mark.parametrize("D,L", [(1, 162), (2, 161), (4, 321), (8, 2100)])
def test_fir_forms_direct_is_autos_fallback(torch_cuda, D, L):
    """AUTO at a tap count only the direct form takes (decim 8: 263 overlap rows, past the
    polyphase-FFT form's 256) -- and the plan it returns runs."""
    torch = torch_cuda
    T = DIRECT_T[D]
    n1, n2 = T + 1, 3
    h, x, hist = make_data("int", L, (n1 + n2) * D, 31 * L + D)
    plan = nsh.FirPlan(h, D, nsh.FIR_AUTO)
    assert plan.algo == nsh.FIR_DIRECT and plan.kernel == direct_name(D), plan.kernel
    chained_calls(torch, plan, "int", h, x, hist, D, n1, n2, "AUTO %s L=%d" % (plan.kernel, L))
    plan.close()


@pytest.mark.parametrize("D", [1, 2, 4, 8])
def test_fir_forms_direct_long_nonfinite(torch_cuda, D):
    """4093 taps (padded to 4096): an inf and a NaN sample, and a NaN in the oldest history sample.
    The NaN / inf pattern equals the oracle's -- the three padded taps must not reach a sample L or
    more back (0 x NaN) -- and the finite outputs meet the tolerance. The bad samples sit where an
    output exists exactly L samples later at every decimation."""
    torch = torch_cuda
    L = 4093
    T = DIRECT_T[D]
    n_out = 2 * T + 3
    h = _firwin(L)
    x = orc.synth(n_out * D, 17 + D)
    hist = orc.synth(L - 1, 10 ** 7 + D)
    i_nan, i_inf = 3, 8 * 40 + 3  # (i + L) % 8 == 0: every decimation has the output at i + L
    x[i_nan] = complex(np.nan, 0.25)
    x[i_inf] = complex(-0.5, np.inf)
    hist[0] = complex(np.nan, np.nan)   # L - 1 back from output 0, L back from input sample 1
    assert (i_nan + L) % 8 == 0 and (i_nan + L) // D < n_out
    plan = nsh.FirPlan(h, D, nsh.FIR_DIRECT)
    assert plan.kernel == direct_name(D), plan.kernel
    y, hout = run_fir(torch, plan, x, n_out, hist=hist)
    ref, href = orc.fir_ccf(x, h, D, hist=hist, return_hist=True)
    _nonfinite_pattern(y, ref)
    nan = np.isnan(ref.real)
    assert nan[0] and nan[(i_nan + L - 1) // D] and not nan[(i_nan + L) // D]  # the case is what it claims
    if D == 1:
        assert not nan[1: i_nan].any()
    fin = np.isfinite(ref.real) & np.isfinite(ref.imag)
    ok, err, scale = orc.tol_ok(y[fin], ref[fin])
    assert ok, (D, err, scale)
    np.testing.assert_array_equal(hout.view(np.uint32), href.view(np.uint32))
    plan.close()
