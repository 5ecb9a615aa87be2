"""nsh_fir_cascade_ccf (k_fir_pfft2<16>, k_fir_pfft<16,1>, k_fir_pfft<8,1>) where tests/test_gpu_pfft.py
cannot see it fail: that file's tap sets are all symmetric windowed-sinc low-passes (time-reversed
taps give the same answer and the composite's outer taps are ~1e-13 of its peak, so a wrong Q, a wrong
first valid row or a lost heq[D Q] passes), and its frames that share a workgroup all carry one scale
exponent and no inf/NaN.

Reference: the composite filter heq composed in float64 from the fp32 stage taps, and
y[m] = sum_n heq[n] x[m D - n] in float64 (FFT convolution; an impulse train is evaluated exactly).
ref64 is checked against the oracle's staged chain without a GPU (test_ref64_matches_oracle_chain). Streams holding inf/NaN are compared with the oracle itself: its staged chain where the plan
runs the stages, oracle.fir_ccf on float32(heq) where the plan runs the composite direct form
(plan_runs_stages restates the rule of nsh_fir_cascade_plan_create).

Tolerance: the contract of include/nsh_hip.h, per output,
    |y - r| <= 1e-5 |r| + 1e-6 lev sum|heq|,   lev = max|x| over the output's frame window,
inputs [D (f V - Q), D (f V - Q) + 512 D) of the call (with its history; finite samples only).
Every test prints and reports its worst error-to-bound ratio (DESIGN.md section 4.2 lists them).

Taps: magnitudes uniform in [0.5, 1] with random signs (asymmetric, every edge tap as large as the
middle ones); multi-stage chains are 2- to 4-tap stages in front of one long stage, sized so that
the stages' taps do not overlap in the composite (every composite tap is one product, none is 0).
Each case asserts its tap margin: min|heq| over the first and last 2 D taps times the input's RMS
is at least 10 times the largest bound.

Group A (taps; a few frames), B (three and four frames per workgroup: per-frame scale exponents on
both sides of every threshold, inf/NaN frames in every position of the three-frame pipeline),
C (plan variants of the non-finite path). The frames-per-workgroup figure is restated from the
device's CU count and asserted. Group B's inf/NaN position cases use Q = 192 (V = 320): at
Q = V = 256 every input row lies in two windows, so no frame can be bad alone; the Q = 256 filter
runs its inf/NaN frames in test_scale_and_nonfinite_together."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from newsched_amd import nsh
from tests.pfft_ref import (CHAINS_A, CHAINS_B, KERNEL16, M, geometry, heq_l1, launch_shape, many_frames_n_out, n_cu_of,  # noqa: F401
                            pfft_form, ref64, ref_chain, run_pfft, taps_u)  # (pfft_form: autouse)

gpu = pytest.mark.gpu
IMG2, MAX_STAGES = 571, 8


# ---------------------------------------------------------------- taps, composite, reference

def plan_runs_stages(stages):
    """nsh_fir_cascade_plan_create's rule: inf/NaN frames run the stages when there are 2 .. 8 of them
    and the first two stage outputs of one window fit a set of phase images; else the direct form on heq."""
    D = int(np.prod([d for _, d in stages]))
    if not 2 <= len(stages) <= MAX_STAGES:
        return False
    n1 = (D * M - 1) // stages[0][1] + 1
    n2 = (n1 - 1) // stages[1][1] + 1
    return n1 + n2 <= D * IMG2


def ref_nonfinite(x, stages):
    """The oracle's answer for a stream holding inf/NaN, by the form the plan runs on such frames."""
    if plan_runs_stages(stages):
        return ref_chain(x, stages)
    heq, D, _, _ = geometry(stages)
    return orc.fir_ccf(x, heq.astype(np.float32), D)


def frame_lev(s, c0, n_out, D, Q, V, L):
    """Per output of a call that starts at sample c0 of stream s (earlier samples: its history, L - 1
    of them) the contract's lev: max|x| over the output's frame window, finite samples only."""
    a = np.abs(np.asarray(s, np.complex128))
    a[~np.isfinite(a)] = 0.0
    end = c0 + D * n_out
    lev = np.empty(n_out)
    for f in range((n_out + V - 1) // V):
        lo = max(c0 + D * (f * V - Q), c0 - (L - 1), 0)
        hi = min(c0 + D * (f * V - Q) + D * M, end)
        lev[f * V:(f + 1) * V] = a[lo:hi].max() if hi > lo else 0.0
    return lev


def bound_ratio(y, r, lev, l1):
    """(worst |y - r| / bound, the bounds, the worst output's index) over the outputs whose reference
    is finite."""
    r = np.asarray(r, np.complex128)
    fin = np.isfinite(r.real) & np.isfinite(r.imag)
    bound = 1e-5 * np.abs(np.where(fin, r, 0)) + 1e-6 * lev * l1
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(np.where(fin, np.asarray(y, np.complex128) - r, 0))
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    assert np.all(np.isfinite(np.asarray(y)[fin].view(np.float32))), "a finite output came out inf/NaN"
    k = int(np.argmax(ratio)) if ratio.size else 0
    return (float(ratio[k]) if ratio.size else 0.0), bound, k


def edge_margin(heq, D, x_rms, bound):
    """min|heq| over the first and last 2 D composite taps, times the input level, over 10 bounds."""
    e = np.abs(np.concatenate([heq[:2 * D], heq[-2 * D:]])).min()
    return float(e * x_rms / (10.0 * bound.max()))


def assert_pattern(y, r, what):
    """NaN positions, inf positions and inf signs per component, exactly."""
    for part in ("real", "imag"):
        a, b = getattr(y, part), getattr(r, part)
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg="%s: NaN positions (%s)" % (what, part))
        np.testing.assert_array_equal(np.isinf(a), np.isinf(b), err_msg="%s: inf positions (%s)" % (what, part))
        np.testing.assert_array_equal(np.sign(a[np.isinf(b)]), np.sign(b[np.isinf(b)]),
                                      err_msg="%s: inf signs (%s)" % (what, part))


def report(what, ratio):
    print("pfft_taps ratio %-44s %.4f" % (what, ratio))


# ---------------------------------------------------------------- the reference itself (CPU)

def test_ref64_matches_oracle_chain():
    """ref64 on a random-tap chain against the oracle's staged chain (double accumulation, fp32
    between the stages): they differ by the chain's fp32 roundings, a small part of the bound."""
    stages = [(taps_u(2, 1), 2), (taps_u(3, 2), 1), (taps_u(301, 3), 4), (taps_u(2, 4), 2)]
    heq, D, Q, V = geometry(stages)
    assert D == 16 and abs(heq_l1(stages) - np.abs(heq).sum()) < 1e-9
    n_out = 2 * V + 5
    s = orc.synth(heq.size - 1 + D * n_out, 17)
    x, hist = s[heq.size - 1:], s[:heq.size - 1]
    r = ref64(x, heq, D, n_out)
    ratio, _, k = bound_ratio(ref_chain(x, stages), r, frame_lev(x, 0, n_out, D, Q, V, heq.size), np.abs(heq).sum())
    assert ratio < 0.05, ratio
    # with a history: the chain over the longer stream
    rh = ref64(x, heq, D, n_out, hist=hist)
    whole = ref_chain(np.concatenate([np.zeros((-s.size) % D, np.complex64), s]), stages)[-n_out:]
    ratio, _, k = bound_ratio(whole, rh, frame_lev(s, heq.size - 1, n_out, D, Q, V, heq.size), np.abs(heq).sum())
    assert ratio < 0.05, ratio
    # the direct sum, at a few outputs
    for m in (0, 1, V, n_out - 1):
        k = np.arange(min(heq.size, m * D + 1))
        assert abs(r[m] - np.sum(heq[k] * x[m * D - k].astype(np.complex128))) < 1e-10 * np.abs(heq).sum()
    # the plan's rule, restated (n1 + n2 against D * 571)
    assert plan_runs_stages([(taps_u(9, 1), 1), (taps_u(200, 2), 16)])
    assert not plan_runs_stages([(taps_u(9, 1), 1), (taps_u(31, 2), 2), (taps_u(200, 3), 8)])
    assert not plan_runs_stages([(taps_u(9, 1), 1), (taps_u(200, 2), 8)])
    assert not plan_runs_stages([(taps_u(100, 1), 16)])


# ---------------------------------------------------------------- group A: taps

@functools.lru_cache(maxsize=None)
def _case_a(name):
    stages = CHAINS_A[name]
    heq, D, Q, V = geometry(stages)
    n = 3 * V + 7
    x = orc.synth(D * n, 100 + len(name))
    return stages, heq, D, Q, V, x, ref64(x, heq, D, n)


@gpu
@pytest.mark.parametrize("name", sorted(CHAINS_A))
def test_asymmetric_taps_vs_float64(torch_cuda, name, pfft_form):
    """Asymmetric full-size taps at the frame shapes: n_out = 1, V - 1, V, V + 1, 3 V + 7 (prefixes of
    one stream), then the stream in three calls (the first exactly one frame, the second cut inside a
    frame) with the history handed on and hist_out compared bit for bit."""
    stages, heq, D, Q, V, x, r = _case_a(name)
    L, l1 = heq.size, np.abs(heq).sum()
    assert np.all(heq != 0.0), "an exactly zero composite tap"
    p = nsh.FirCascadePlan(stages)
    assert p.decim == D and p.hist_len == L - 1
    assert p.kernel == (KERNEL16[pfft_form] if D == 16 else "k_fir_pfft<8,1>")
    assert (Q, V) == ((L - 1 + D - 1) // D, M - Q) and Q <= 256
    worst = 0.0
    for n_out in (1, V - 1, V, V + 1, 3 * V + 7):
        xs = x[:D * n_out]
        y, hout = run_pfft(torch_cuda, p, xs, n_out)
        ratio, bound, k = bound_ratio(y, r[:n_out], frame_lev(xs, 0, n_out, D, Q, V, L), l1)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, n_out, ratio, k)
        np.testing.assert_array_equal(hout, np.concatenate([np.zeros(L - 1, np.complex64), xs])[xs.size:])
    assert edge_margin(heq, D, float(np.sqrt(np.mean(np.abs(x) ** 2))), bound) >= 1.0, "tap margin"
    cuts = [0, V, V + V // 2 + 1, 3 * V + 7]
    hist = None
    for a, b in zip(cuts[:-1], cuts[1:]):
        y, hist = run_pfft(torch_cuda, p, x[D * a:D * b], b - a, hist)
        lev = frame_lev(x, D * a, b - a, D, Q, V, L)
        ratio, _, k = bound_ratio(y, r[a:b], lev, l1)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, "split", a, b, ratio)
        np.testing.assert_array_equal(hist, np.concatenate([np.zeros(L - 1, np.complex64), x[:D * b]])[D * b:])
    report("A.taps %s %s" % (name, pfft_form), worst)


IMPULSE_CHAINS = {"d16-L4097-q256": CHAINS_A["d16-L4097-q256"], "d16-2x8": CHAINS_A["d16-2x8"],
                  "d8-L2049-q256": CHAINS_A["d8-L2049-q256"]}


@functools.lru_cache(maxsize=None)
def _case_impulse(name):
    stages = IMPULSE_CHAINS[name]
    heq, D, Q, V = geometry(stages)
    L = heq.size
    step = V * ((V + 2 * Q + 2 + V - 1) // V)  # rows between impulses: the responses stay apart
    # (row of its region's first frame, phase): every phase of one row, then the rows at which a
    # response meets the frame edges
    spots = [(3, ph) for ph in range(D)] + [(row, D - 1 - row % D) for row in (0, Q - 1, Q, V - 1, V, V + Q)]
    t0 = [D * (k * step + row) + ph for k, (row, ph) in enumerate(spots)]
    n_out = (len(spots) + 1) * step - 7
    t0 += [D * (n_out - 1), D * n_out - 1]  # the last row's first sample (y[n_out - 1] = heq[0]); the last input (no output)
    x = np.zeros(D * n_out, np.complex64)
    x[t0] = 1.0
    r = np.zeros(n_out)
    inside = np.zeros(n_out, bool)
    m = np.arange(n_out)
    for t in t0:
        k = m * D - t
        ok = (k >= 0) & (k < L)
        r[ok] += heq[k[ok]]
        inside |= ok
    assert np.all(np.diff(t0[:-1]) > L)
    return stages, heq, D, Q, V, x, r, inside, n_out


@gpu
@pytest.mark.parametrize("name", sorted(IMPULSE_CHAINS))
def test_impulse_responses(torch_cuda, name, pfft_form):
    """Unit impulses at every phase of a row, at the rows where the response meets a frame edge (rows
    0, Q - 1, Q, V - 1, V, V + Q of a frame) and at the call's last input, one launch: the output is
    heq[m D - t0], tap by tap, and within the bound of zero outside every response."""
    stages, heq, D, Q, V, x, r, inside, n_out = _case_impulse(name)
    l1 = np.abs(heq).sum()
    assert np.all(heq != 0.0)
    p = nsh.FirCascadePlan(stages)
    y, _ = run_pfft(torch_cuda, p, x, n_out, want_hist=False)
    ratio, bound, k = bound_ratio(y, r, frame_lev(x, 0, n_out, D, Q, V, heq.size), l1)
    assert edge_margin(heq, D, 1.0, bound) >= 1.0, "tap margin"
    assert inside.sum() >= 10 * Q and (~inside).sum() > n_out // 2
    assert np.all(np.abs(y.imag) <= bound), "a real impulse through real taps"
    assert ratio <= 1.0, (name, ratio, k, bool(inside[k]))
    report("A.impulse %s %s" % (name, pfft_form), ratio)


@gpu
@pytest.mark.parametrize("algo", [nsh.FIR_AUTO, nsh.FIR_PFFT], ids=["auto", "pfft"])
@pytest.mark.parametrize("decim,ntaps", [(8, 301), (16, 705)])
def test_firplan_asymmetric_taps(torch_cuda, decim, ntaps, algo, pfft_form):
    """nsh.FirPlan (AUTO and NSH_FIR_PFFT) on asymmetric taps, a stream in calls with the ntaps - 1
    history handed on: test_firplan_auto_pfft's contract on taps that a reversal fails."""
    torch = torch_cuda
    h = taps_u(ntaps, 7 * decim)
    heq, D, Q, V = geometry([(h, decim)])
    plan = nsh.FirPlan(h, decim, algo)
    assert plan.algo == nsh.FIR_PFFT and plan.kernel == (KERNEL16[pfft_form] if decim == 16 else "k_fir_pfft<8,1>")
    cuts = [0, 3, V, V + 1, 3 * V + 50]
    x = orc.synth(decim * cuts[-1], ntaps)
    r = ref64(x, heq, D, cuts[-1])
    hist = torch.zeros(ntaps - 1, dtype=torch.complex64, device="cuda")
    hout = torch.zeros_like(hist)
    worst = 0.0
    for a, b in zip(cuts[:-1], cuts[1:]):
        dx = torch.from_numpy(x[decim * a:decim * b]).cuda()
        dy = torch.empty(b - a, dtype=torch.complex64, device="cuda")
        plan(dx, hist if a else 0, hout, dy, b - a)
        torch.cuda.synchronize()
        hist, hout = hout, hist
        ratio, bound, k = bound_ratio(dy.cpu().numpy(), r[a:b], frame_lev(x, decim * a, b - a, D, Q, V, ntaps), np.abs(heq).sum())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (decim, ntaps, a, b, ratio)
        np.testing.assert_array_equal(hist.cpu().numpy(), np.concatenate([np.zeros(ntaps - 1, np.complex64), x[:decim * b]])[decim * b:])
    assert edge_margin(heq, D, float(np.sqrt(np.mean(np.abs(x) ** 2))), bound) >= 1.0, "tap margin"
    report("A.firplan d%d %s" % (decim, pfft_form), worst)


# ---------------------------------------------------------------- group B: many frames per workgroup

# scale exponent of each run of two frames' new rows (cut at D f V), cyclic: equal and different
# neighbours, both sides of the +-40 scaling threshold and of form 2's pass-1 re-do thresholds
# (frame maximum >= 2^124, < 2^-100)
EXPONENTS = (0, 60, -60, 125, -110, 0)

MIN_FPW = {16: 4, 8: 3}


def assert_many_frames(n_out, V, D, n_cu):
    nf, fpw, wgs = launch_shape(n_out, V, D, n_cu)
    assert fpw >= MIN_FPW[D], (nf, fpw)
    assert 0 < nf - (wgs - 1) * fpw < fpw, "the last workgroup is short"
    return nf, fpw, wgs


def ref64_runs(x0, heq, D, n_out, run_len, e_run):
    """ref64 of x0 * 2^e, e constant over runs of run_len samples (run k: e_run[k]), without mixing
    magnitudes 2^235 apart in one transform: runs two-coloured, one convolution per colour (an output
    meets at most one run of each colour, as len(heq) - 1 <= run_len), each scaled by its run's 2^e."""
    L = heq.size
    assert L - 1 <= run_len
    run = np.arange(x0.size) // run_len
    xa = np.where(run % 2 == 0, x0, 0).astype(np.complex128)
    ya, yb = ref64(xa, heq, D, n_out), ref64(x0.astype(np.complex128) - xa, heq, D, n_out)
    m = np.arange(n_out)
    hi, lo = (m * D) // run_len, np.maximum(m * D - (L - 1), 0) // run_len
    e = np.asarray(e_run, np.float64)
    r = np.zeros(n_out, np.complex128)
    for colour, yc in ((0, ya), (1, yb)):
        k = np.where(hi % 2 == colour, hi, lo)
        r += np.where(k % 2 == colour, yc * 2.0 ** e[k], 0)
    return r


@functools.lru_cache(maxsize=None)
def _case_scale(name, n_cu):
    stages = CHAINS_B[name]
    heq, D, Q, V = geometry(stages)
    n_out = many_frames_n_out(V, D, n_cu)
    x0 = orc.synth(D * n_out, 7)
    run_len = 2 * V * D
    n_runs = (x0.size + run_len - 1) // run_len
    e_run = np.array([EXPONENTS[k % len(EXPONENTS)] for k in range(n_runs)])
    x = (x0.astype(np.complex128) * 2.0 ** np.repeat(e_run, run_len)[:x0.size]).astype(np.complex64)
    assert np.all(x.astype(np.complex128) == x0.astype(np.complex128) * 2.0 ** np.repeat(e_run, run_len)[:x0.size])
    r = ref64_runs(x0, heq, D, n_out, run_len, e_run)
    r.setflags(write=False)
    return stages, heq, D, Q, V, n_out, x, r, e_run


@gpu
@pytest.mark.parametrize("name", ["d16-L4097", "d8-L2049", "c5"])
def test_per_frame_scale_many_frames(torch_cuda, name, pfft_form):
    """Four (D = 8: three) frames per workgroup, the input times 2^e with e from EXPONENTS constant
    over two frames' new rows: each frame is held to the contract at its own window's level, so a scale
    taken from a neighbouring frame (wrong by 2^50 or more) cannot pass."""
    n_cu = n_cu_of(torch_cuda)
    stages, heq, D, Q, V, n_out, x, r, e_run = _case_scale(name, n_cu)
    nf, fpw, wgs = assert_many_frames(n_out, V, D, n_cu)
    l1 = np.abs(heq).sum()
    amax = float(np.abs(x).max())
    assert amax * l1 < 3.0e38 and amax >= 2.0 ** 124  # inside fp32; form 2's re-do threshold reached
    # inside one workgroup: equal and different neighbouring exponents
    e_frame = e_run[np.arange(nf) // 2]
    per_wg = [e_frame[b * fpw:(b + 1) * fpw] for b in range(wgs - 1)]
    assert any(np.any(np.diff(e) == 0) and np.any(np.diff(e) != 0) for e in per_wg)
    p = nsh.FirCascadePlan(stages)
    y, _ = run_pfft(torch_cuda, p, x, n_out, want_hist=False)
    ratio, _, k = bound_ratio(y, r, frame_lev(x, 0, n_out, D, Q, V, heq.size), l1)
    assert ratio <= 1.0, (name, ratio, "frame", k // V, "of", nf, "fpw", fpw)
    report("B.scale %s %s" % (name, pfft_form), ratio)


# good/bad frames of one workgroup (four frames at D = 16); at three frames per workgroup (D = 8)
# the first three letters are used
PATTERNS = ("BGGG", "GBGG", "GGBG", "GGGB", "GGBB", "BBGG", "BBBB", "GBGB")
BAD_VALUES = (complex(np.nan, 0.25), complex(np.inf, -0.5), complex(-0.75, -np.inf), complex(-np.inf, np.nan))


def plant_bad_frames(x, D, Q, V, nf, fpw, wgs):
    """inf/NaN samples in rows that only their own frame's window holds (the first V - Q new rows of
    frame f), so that workgroups 2, 5, 8, ... show PATTERNS; one sample in the overlap rows shared by
    two frames; the short last workgroup's last frame. Returns the frames made bad."""
    assert V - Q >= 16 and wgs > 3 * len(PATTERNS) + 8
    bad = set()
    n = 0
    for k, pat in enumerate(PATTERNS):
        b = 2 + 3 * k
        for i, c in enumerate(pat[:fpw]):
            if c == "B":
                f = b * fpw + i
                x[D * (f * V + 5 + n % 7) + n % D] = BAD_VALUES[n % len(BAD_VALUES)]
                bad.add(f)
                n += 1
    f = (4 + 3 * len(PATTERNS)) * fpw + 1  # overlap rows of frames f and f + 1: both bad
    x[D * ((f + 1) * V - Q // 2) + 1] = complex(np.inf, 1.0)
    x[D * ((f + 1) * V - Q // 2) + 9] = complex(-np.inf, 1.0)
    bad |= {f, f + 1}
    x[D * (x.size // D - 1)] = complex(np.nan, np.inf)  # the last output's newest row: the launch's last frame
    bad.add(nf - 1)
    return bad


def assert_bad_frames(r, bad, V, nf):
    """The reference holds non-finite outputs in exactly the bad frames, and finite ones in each of
    them that has more than a few outputs."""
    fin = np.isfinite(r.real) & np.isfinite(r.imag)
    frames = set((np.flatnonzero(~fin) // V).tolist())
    assert frames == bad, (sorted(frames ^ bad))
    for f in bad:
        if min((f + 1) * V, r.size) - f * V > 8:
            assert fin[f * V:(f + 1) * V].any(), f


@functools.lru_cache(maxsize=None)
def _case_nonfinite(name, n_cu):
    stages = CHAINS_B[name]
    heq, D, Q, V = geometry(stages)
    n_out = many_frames_n_out(V, D, n_cu)
    nf, fpw, wgs = launch_shape(n_out, V, D, n_cu)
    x = orc.synth(D * n_out, 9)
    bad = plant_bad_frames(x, D, Q, V, nf, fpw, wgs)
    r = ref_nonfinite(x, stages)
    r.setflags(write=False)
    return stages, heq, D, Q, V, n_out, x, r, bad


@gpu
@pytest.mark.parametrize("name", ["d16-L3073", "d16-2x8-q192", "d8-L1537", "d8-2x4-q192", "c5"])
def test_nonfinite_frames_in_every_pipeline_position(torch_cuda, name, pfft_form):
    """inf/NaN frames first, second, third and last in a workgroup, in pairs, alternating, a whole
    workgroup, the short last workgroup, and a sample in the rows two frames share: the NaN and inf
    outputs are the oracle's exactly (the staged chain for the chains, the direct form for single
    stages) and every finite output -- the good frames beside the bad ones -- is within the bound."""
    n_cu = n_cu_of(torch_cuda)
    stages, heq, D, Q, V, n_out, x, r, bad = _case_nonfinite(name, n_cu)
    nf, fpw, wgs = assert_many_frames(n_out, V, D, n_cu)
    assert plan_runs_stages(stages) == (len(stages) > 1)
    assert np.all(heq != 0.0)
    assert_bad_frames(r, bad, V, nf)
    p = nsh.FirCascadePlan(stages)
    y, _ = run_pfft(torch_cuda, p, x, n_out, want_hist=False)
    assert_pattern(y, r, name)
    ratio, _, k = bound_ratio(y, r, frame_lev(x, 0, n_out, D, Q, V, heq.size), np.abs(heq).sum())
    assert ratio <= 1.0, (name, ratio, "frame", k // V, "in workgroup", k // V // fpw, "fpw", fpw)
    report("B.nonfinite %s %s" % (name, pfft_form), ratio)


@functools.lru_cache(maxsize=None)
def _case_both(name, n_cu):
    stages, heq, D, Q, V, n_out, xs, _, e_run = _case_scale(name, n_cu)
    nf, fpw, wgs = launch_shape(n_out, V, D, n_cu)
    assert fpw == 4
    x = xs.copy()
    bad, between = set(), []
    for k, b in enumerate(range(1, 1 + 2 * len(EXPONENTS))):
        # frame 4 b + 1 ends a run of one exponent, frame 4 b + 2 starts the next. A sample in its first
        # new rows: at Q < V only its own window holds them, at Q = V the next frame's does too
        f = b * fpw + 1
        x[D * (f * V + 3) + k % D] = BAD_VALUES[k % len(BAD_VALUES)]
        frames = [f] if Q < V - 3 else [f, f + 1]
        bad |= set(frames)
        between.append((f - 1, frames[-1] + 1))  # the good frames on either side
    r = ref_nonfinite(x, stages)
    r.setflags(write=False)
    return stages, heq, D, Q, V, n_out, x, r, bad, between, e_run


@gpu
@pytest.mark.parametrize("name", ["d16-L4097", "c5"])
def test_scale_and_nonfinite_together(torch_cuda, name, pfft_form):
    """inf/NaN frames between frames of different scale exponents (every neighbouring pair of
    EXPONENTS), four frames per workgroup."""
    n_cu = n_cu_of(torch_cuda)
    stages, heq, D, Q, V, n_out, x, r, bad, between, e_run = _case_both(name, n_cu)
    nf, fpw, wgs = assert_many_frames(n_out, V, D, n_cu)
    assert_bad_frames(r, bad, V, nf)
    e_frame = e_run[np.arange(nf) // 2]
    assert sum(e_frame[a] != e_frame[b] for a, b in between) >= len(EXPONENTS)
    assert all(a // fpw == b // fpw and a not in bad and b not in bad for a, b in between)  # one workgroup
    p = nsh.FirCascadePlan(stages)
    y, _ = run_pfft(torch_cuda, p, x, n_out, want_hist=False)
    assert_pattern(y, r, name)
    ratio, _, k = bound_ratio(y, r, frame_lev(x, 0, n_out, D, Q, V, heq.size), np.abs(heq).sum())
    assert ratio <= 1.0, (name, ratio, "frame", k // V, "fpw", fpw)
    report("B.both %s %s" % (name, pfft_form), ratio)


# ---------------------------------------------------------------- group C: plan variants of the non-finite path

def _two(seed, d):
    return (taps_u(2, seed), d)


PLANS_C = {
    "d1-d16": [(taps_u(9, 71), 1), (taps_u(200, 72), 16)],                       # 8192 + 512 fits: stages
    "d1-d2-d8": [(taps_u(9, 73), 1), (taps_u(31, 74), 2), (taps_u(200, 75), 8)],  # 8192 + 4096 does not
    "d1-d8": [(taps_u(9, 76), 1), (taps_u(200, 77), 8)],                          # D = 8: 4096 + 512 does not
    "nine-stages": [_two(80 + k, 1) for k in range(5)] + [_two(85 + k, 2) for k in range(3)] + [(taps_u(40, 89), 2)],
    "eight-stages": [_two(90, 2)] + [_two(91 + k, 1) for k in range(4)] + [_two(95, 2), _two(96, 2), (taps_u(40, 97), 2)],
    "eight-stages-d1-first": [_two(100 + k, 1) for k in range(4)] + [_two(104 + k, 2) for k in range(3)] + [(taps_u(40, 107), 2)],
    "single": [(taps_u(200, 78), 16)],
}
STAGED_C = {"d1-d16": True, "d1-d2-d8": False, "d1-d8": False, "nine-stages": False, "eight-stages": True,
            "eight-stages-d1-first": False, "single": False}


@functools.lru_cache(maxsize=None)
def _case_c(name):
    stages = PLANS_C[name]
    heq, D, Q, V = geometry(stages)
    n_out = 3 * V + 5
    x = orc.synth(D * n_out, 13)
    at = D * (V + 40)  # frame 1 (and frame 0's last rows see nothing of it)
    x[at] = complex(np.nan, 0.5)
    x[at + 3 * D * Q + 2] = complex(np.inf, -0.5)
    x[at + 3 * D * Q + 5] = complex(-np.inf, np.inf)
    x[at + 3 * D * Q + 6] = complex(0.5, -np.inf)
    staged, comp = ref_chain(x, stages), orc.fir_ccf(x, heq.astype(np.float32), D)
    return stages, heq, D, Q, V, n_out, x, staged, comp


@gpu
@pytest.mark.parametrize("name", sorted(PLANS_C))
def test_nonfinite_plan_variants(torch_cuda, name, pfft_form):
    """Plans on both sides of the rule that picks the non-finite path (2 .. 8 stages whose first two
    outputs fit the image sets run the stages; the others, a leading decimation-1 stage that does not
    fit and nine stages among them, the direct form on heq): +inf and -inf three samples apart give the
    chain's inf - inf = NaN in the first case and the composite's +-inf in the second."""
    stages, heq, D, Q, V, n_out, x, staged, comp = _case_c(name)
    assert plan_runs_stages(stages) == STAGED_C[name]
    assert np.all(heq != 0.0) and Q <= 256
    r = staged if STAGED_C[name] else comp
    if len(stages) > 1:  # the two forms differ on this input: the case tells them apart
        assert not (np.array_equal(np.isnan(staged.view(np.float32)), np.isnan(comp.view(np.float32)))
                    and np.array_equal(np.isinf(staged.view(np.float32)), np.isinf(comp.view(np.float32))))
    fin = np.isfinite(r.real) & np.isfinite(r.imag)
    assert (~fin).any() and all(fin[f * V:(f + 1) * V].any() for f in set((np.flatnonzero(~fin) // V).tolist()))
    p = nsh.FirCascadePlan(stages)
    y, _ = run_pfft(torch_cuda, p, x, n_out, want_hist=False)
    assert_pattern(y, r, name)
    ratio, _, k = bound_ratio(y, r, frame_lev(x, 0, n_out, D, Q, V, heq.size), np.abs(heq).sum())
    assert ratio <= 1.0, (name, ratio)
    report("C.plan %s %s" % (name, pfft_form), ratio)
