"""The accuracy gate of nsh_fir_cascade_ccf (k_fir_pfft2<16>, k_fir_pfft<16,1>, k_fir_pfft<8,1>): the
polyphase-FFT overlap-save FIR held to the rms error of a complex64 model of its own algorithm, over
the whole call and at its worst position (tests/fft_accuracy.py: whole <= 1.25 x model, worst <= 1.5 x
model, at least 64 frames per position and 2^16 outputs).

tests/test_gpu_pfft.py and tests/test_gpu_pfft_taps.py end in oracle.tol_ok at 1e-5 or in the header's
per-output bound, which a correct kernel meets thirty times over: a twiddle with six digits, tables
from fp32 angles, one wave's constants wrong all pass them. They do not pass here.

Model: pfft_ref.pfft_model -- the windows, P phase sequences of 512, scipy.fft in complex64, times
F_p = FFT_512(g_p) / 512 (double, rounded once), the phase sum in complex64 in ascending p, the
unnormalised inverse. Reference: pfft_ref.ref64, the float64 composite filter on the fp32 inputs (the
oracle's staged chain rounds to fp32 between stages, about as much as the kernel errs in all).
Inputs: gpu_util.uniform with a nonzero history of len(heq) - 1 samples.

Two layouts of the same gate:
  A  position = output row q of a frame (V of them), frames_for(V) frames. One workgroup per frame.
  B  position = (k, q), k the frame's index inside its workgroup: 8 frames in every workgroup, as many
     workgroups as the device runs at once (restated from its CU count and asserted). f & 3 == k & 3 and
     f & 1 == k & 1, so one inverse wave or one image set gone wrong stays at its own positions; k = 0
     is a workgroup's first-frame load path, k = 7 its drain; the pipelined steady state runs at all.

The CPU tests (not marked gpu) prove per chain that the gate discriminates. A radix-2 complex64
chain with exact tables and a reversed phase sum pass (SPREAD lines); the planted defects (DEFECT
lines) fail a gate or are listed in NOT_VISIBLE and then asserted to pass. Ratios to the model:
(the model's own figures: 1.68e-7 to 1.77e-7 whole, 1.91e-7 to 2.03e-7 worst)
                                             c5             d16-L4097      d16-L7         d8-L2049
  radix-2, exact tables                      1.019 / 1.104  1.023 / 1.029  1.015 / 1.042  1.027 / 1.034
  phase sum descending                       0.999 / 0.983  1.002 / 0.978  1.006 / 0.995  1.002 / 0.967
  one inverse-table entry x (1 + 1e-6)       1.038 / 3.548  1.051 / 3.494  1.048 / 3.585  1.059 / 3.753
  fp32 angles in both tables                 1.252 / 1.629  1.262 / 1.442  1.229 / 1.892  1.292 / 1.501
  the largest F entry x (1 + 1e-5)           1.181 / 1.150* 2.428 / 2.235  1.544 / 1.476  2.861 / 2.638
  last composite tap lost                    1.000 / 1.000* 8.5e4 / 7.9e4  2.1e6 / 1.9e6  9.7e4 / 8.9e4
  one forward-table entry x (1 + 1e-6)*      1.053 / 1.136  1.052 / 1.076  1.044 / 1.069  1.076 / 1.081
  the largest F entry x (1 + 1e-6)*          1.002 / 0.999  1.026 / 1.017  1.005 / 0.993  1.036 / 1.008
  F from fp32-rounded heq*                   1.011 / 1.009  1.000 / 1.000  1.000 / 1.000  1.000 / 1.000
  (* not visible: C5's last composite tap is 1e-13 of its peak and its pass band holds many F entries of
  the largest one's size; a forward-table error spreads evenly over the output rows.)
  The inverse-entry defect on some frames only, layout A | layout B, worst position:
    frames f & 3 == 1 (one inverse wave)     c5 1.934 | 3.190    d8-L2049 1.877 | 2.947   (both layouts fail)
    frames f % 16 == 5 (half of k = 5)       c5 1.266 | 2.322    d8-L2049 1.277 | 2.235   (only B fails)

test_scale_is_exact: the source's claim that the per-frame power-of-two scale changes no output bit,
as a metamorphic test: the outputs of x0 2^e are those of x0 times 2^e, bit for bit, for e on both
sides of the scale threshold and of form 2's pass-1 re-do thresholds.

Measured on one MI355X (profiles/pfft_accuracy_ratios.log; kernel, model, kernel / model;
every case passes; no kernel needed a change and no model an extension)
                                          whole                           worst position
  A c5         pfft2<16> | pfft<16,1>     1.72e-7 1.77e-7 0.969 | 0.964   1.96e-7 2.03e-7 0.962 | 0.935
  A d16-L4097  pfft2<16> | pfft<16,1>     1.72e-7 1.77e-7 0.972 | 0.972   1.92e-7 2.02e-7 0.955 | 0.955
  A d16-L7     pfft2<16> | pfft<16,1>     1.62e-7 1.68e-7 0.966 | 0.965   1.91e-7 2.01e-7 0.954 | 0.903
  A d16-2x8    pfft2<16> | pfft<16,1>     1.72e-7 1.77e-7 0.970 | 0.972   1.98e-7 2.03e-7 0.975 | 0.962
  A d8-L2049   pfft<8,1>                  1.64e-7 1.68e-7 0.974           1.86e-7 1.91e-7 0.974
  A d8-2x4     pfft<8,1>                  1.64e-7 1.69e-7 0.971           1.80e-7 1.91e-7 0.944
  B c5         pfft2<16> | pfft<16,1>     1.71e-7 1.77e-7 0.969 | 0.969   1.93e-7 2.01e-7 0.961 | 0.957
  B d8-L2049   pfft<8,1>, 512 workgroups  1.63e-7 1.69e-7 0.967           1.81e-7 1.87e-7 0.968
(kernel and model figures of the first form; 256 CUs.) The kernel is a little better than the model, as
its radix-8 passes round less often than scipy's and cmul_asm's products are fused.
test_scale_is_exact: bit-equal in all 24 runs (3 plans, 2 forms, 4 exponents; C5 fits fp32 at 2^125 too);
left out as subnormal at e = -110: 0.013 % (C5), 0.084 % (L = 4097), 0.059 % (L = 2049) of the components,
none at the other exponents.
Mutation check (scratch builds): with R2 of dft8 shortened to 0.707107f all 16 gate cases fail (3.4 to
3.8 in whole, 3.5 to 5.3 in worst) while tests/test_gpu_pfft.py and test_gpu_pfft_taps.py stay green (260
passed); with wave 5's t3[3] times 1 + 1e-6 in k_fir_pfft2, layout B on C5 fails (1.40 whole, 2.23 worst)
and so do the four D = 16 cases of layout A on that form (1.35 to 1.40 whole; C5 1.61 worst), through
the wave's forward transform of phase 5, which uses the same constant."""
import functools

import numpy as np
import pytest

from newsched_amd import nsh
from tests import fft_accuracy as acc
from tests.fft_accuracy import fft_r2, table_exact, table_fp32_angles, table_one_entry_off
from tests.gpu_util import bits, first_mismatch, int_signal, uniform
from tests.pfft_ref import (C5, CHAINS_A, CHAINS_B, KERNEL16, M, by_workgroup, geometry, heq_l1, image_table,  # noqa: F401
                            launch_shape, many_frames_n_out, n_cu_of, pfft_form, pfft_model, ref64, run_pfft,
                            taps_u)  # (pfft_form: autouse)

gpu = pytest.mark.gpu

CHAINS = {
    "c5": C5,                                        # Q = 119
    "d16-L4097": CHAINS_A["d16-L4097-q256"],         # Q = V = 256
    "d16-L7": [(taps_u(7, 1007), 16)],               # Q = 1, V = 511
    "d8-L2049": CHAINS_A["d8-L2049-q256"],
    "d16-2x8": CHAINS_A["d16-2x8"],
    "d8-2x4": CHAINS_A["d8-2x4"],
}
FPW = 8  # layout B: frames per workgroup


def kernel_of(D, form):
    return KERNEL16[form] if D == 16 else "k_fir_pfft<8,1>"


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case_a(name):
    """Layout A: inputs, reference and model of a chain, once (both forms and the CPU tests share them)."""
    stages = CHAINS[name]
    heq, D, Q, V = geometry(stages)
    frames = acc.frames_for(V)
    n_out = frames * V
    x, hist = uniform(D * n_out, 900 + len(name)), uniform(heq.size - 1, 901)
    r, model = ref64(x, heq, D, n_out, hist), pfft_model(x, hist, stages, n_out)
    _freeze(x, hist, r, model)
    return stages, heq, D, Q, V, frames, n_out, x, hist, r, model


@functools.lru_cache(maxsize=None)
def case_b(name, max_wg):
    """Layout B: FPW frames in each of max_wg workgroups."""
    stages = CHAINS[name]
    heq, D, Q, V = geometry(stages)
    n_out = FPW * max_wg * V
    x, hist = uniform(D * n_out, 950 + len(name)), uniform(heq.size - 1, 951)
    r, model = ref64(x, heq, D, n_out, hist), pfft_model(x, hist, stages, n_out)
    _freeze(x, hist, r, model)
    return stages, heq, D, Q, V, n_out, x, hist, r, model


# ---- CPU: what the gate lets through and what it does not, per chain -----------------------------------
CPU_CHAINS = ["c5", "d16-L4097", "d16-L7", "d8-L2049"]


def r2(table, inverse=False):
    return lambda a: fft_r2(a, table, inverse)


def entry_off(F, factor):
    """The image table with its largest entry times `factor`."""
    G = F.copy()
    k = np.unravel_index(int(np.argmax(np.abs(F))), F.shape)
    G[k] = np.complex64(np.complex128(G[k]) * factor)
    assert G[k] != F[k]
    return G


def last_tap_lost(stages):
    heq = geometry(stages)[0].copy()
    assert heq[-1] != 0.0
    heq[-1] = 0.0
    return image_table(stages, heq)


def variants(name):
    """(correct, defects) of a chain: what -> pfft_model's keyword arguments."""
    stages = CHAINS[name]
    F, P = image_table(stages), geometry(stages)[1]
    exact, off, ang = table_exact(M), table_one_entry_off(M), table_fp32_angles(M)
    correct = {"radix-2, exact tables": dict(fwd=r2(exact), inv=r2(exact, True)),
               "phase sum descending": dict(order=range(P - 1, -1, -1))}
    defects = {"one inverse-table entry x (1 + 1e-6)": dict(fwd=r2(exact), inv=r2(off, True)),
               "fp32 angles in both tables": dict(fwd=r2(ang), inv=r2(ang, True)),
               "one F entry x (1 + 1e-5)": dict(F=entry_off(F, 1.0 + 1e-5)),
               "last composite tap lost": dict(F=last_tap_lost(stages)),
               "one forward-table entry x (1 + 1e-6)": dict(fwd=r2(off), inv=r2(exact, True)),
               "one F entry x (1 + 1e-6)": dict(F=entry_off(F, 1.0 + 1e-6)),
               "F from fp32-rounded heq": dict(F=image_table(stages, geometry(stages)[0].astype(np.float32)))}
    return correct, defects


# defects inside the spread of the correct variants on that chain: asserted to pass, so the list stays true
NOT_VISIBLE = {(c, d) for c in CPU_CHAINS for d in ("one forward-table entry x (1 + 1e-6)", "one F entry x (1 + 1e-6)",
                                                    "F from fp32-rounded heq")}
NOT_VISIBLE |= {("c5", "last composite tap lost"), ("c5", "one F entry x (1 + 1e-5)")}
# what the issue of this gate requires to be seen
MUST_FAIL = {(c, d) for c in CPU_CHAINS for d in ("one inverse-table entry x (1 + 1e-6)", "fp32 angles in both tables")}
MUST_FAIL |= {("d8-L2049", "one F entry x (1 + 1e-5)"), ("d16-L4097", "last composite tap lost"),
              ("d8-L2049", "last composite tap lost")}


def ratios(y, model, r, frames):
    (wk, pk), (wm, pm) = acc.stats(y, r, frames), acc.stats(model, r, frames)
    return wk / wm, pk / pm


@pytest.mark.parametrize("name", CPU_CHAINS)
def test_cpu_correct_variants_pass(name):
    """A second correct fp32 implementation of the chain passes against the model."""
    stages, heq, D, Q, V, frames, n_out, x, hist, r, model = case_a(name)
    wm, pm = acc.stats(model, r, frames)
    print("MODEL %s: whole %.3g worst %.3g" % (name, wm, pm))
    for what, kw in variants(name)[0].items():
        y = pfft_model(x, hist, stages, n_out, **kw)
        print("SPREAD %s: %s: whole %.3f worst %.3f" % ((name, what) + ratios(y, model, r, frames)))
        acc.gate("%s model, %s" % (name, what), y, model, r, frames)


@pytest.mark.parametrize("name", CPU_CHAINS)
def test_cpu_defects_fail(name):
    """Every planted defect fails at least one of the two gates, or is listed as not visible on that
    chain -- and then does pass."""
    stages, heq, D, Q, V, frames, n_out, x, hist, r, model = case_a(name)
    assert not NOT_VISIBLE & MUST_FAIL
    for what, kw in variants(name)[1].items():
        y = pfft_model(x, hist, stages, n_out, **kw)
        hidden = (name, what) in NOT_VISIBLE
        print("DEFECT %s: %s: whole %.3f worst %.3f%s"
              % ((name, what) + ratios(y, model, r, frames) + (" (not visible to this gate)" if hidden else "",)))
        if hidden:
            acc.gate("%s model, %s" % (name, what), y, model, r, frames)
        else:
            with pytest.raises(AssertionError, match="whole|worst position"):
                acc.gate("%s model, %s" % (name, what), y, model, r, frames)


@functools.lru_cache(maxsize=None)
def one_wave_case(name):
    """Layout B's case at 64 workgroups with the radix-2 chain's outputs, exact and with one
    inverse-table entry times 1 + 1e-6."""
    c = case_b(name, 64)
    stages, n_out, x, hist = c[0], c[5], c[6], c[7]
    good = pfft_model(x, hist, stages, n_out, fwd=r2(table_exact(M)), inv=r2(table_exact(M), True))
    bad = pfft_model(x, hist, stages, n_out, fwd=r2(table_exact(M)), inv=r2(table_one_entry_off(M), True))
    return c, good, bad


# (frames that carry the defect, does layout A's gate see it too)
SOME_FRAMES = {"f & 3 == 1": (lambda f: f & 3 == 1, True), "f % 16 == 5": (lambda f: f % 16 == 5, False)}


@pytest.mark.parametrize("which", list(SOME_FRAMES))
@pytest.mark.parametrize("name", ["c5", "d8-L2049"])
def test_cpu_defect_on_some_frames_needs_layout_b(name, which):
    """One inverse-table entry times 1 + 1e-6 on some frames only. On the frames of one of the four
    inverse waves (f & 3 == 1) it fails layout B's worst position, where those frames have positions of
    their own (k = 1 and 5); three clean frames in four bring it down to 1.9 x the model in layout A,
    still outside. On one frame in sixteen (half of the frames at k = 5) layout A lets it pass and
    layout B does not: why the second layout exists."""
    (stages, heq, D, Q, V, n_out, x, hist, r, model), good, bad = one_wave_case(name)
    on, seen_in_a = SOME_FRAMES[which]
    y = np.where(on(np.arange(n_out) // V), bad, good)
    what = "%s model, one inverse entry x (1 + 1e-6) on frames %s" % (name, which)
    print("DEFECT %s: layout A whole %.3f worst %.3f" % ((what,) + ratios(y, model, r, FPW * 64)))
    if seen_in_a:
        with pytest.raises(AssertionError, match="worst position"):
            acc.gate(what + ", layout A", y, model, r, FPW * 64)
    else:
        acc.gate(what + ", layout A", y, model, r, FPW * 64)
    (yb, frames), (mb, _), (rb, _) = by_workgroup(y, FPW, V), by_workgroup(model, FPW, V), by_workgroup(r, FPW, V)
    assert frames == 64
    print("DEFECT %s: layout B whole %.3f worst %.3f" % ((what,) + ratios(yb, mb, rb, frames)))
    with pytest.raises(AssertionError, match="worst position"):
        acc.gate(what + ", layout B", yb, mb, rb, frames)


# ---- GPU ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", list(CHAINS))
def test_layout_a(torch_cuda, name, pfft_form):
    """Position = output row q; one frame per workgroup."""
    stages, heq, D, Q, V, frames, n_out, x, hist, r, model = case_a(name)
    p = nsh.FirCascadePlan(stages)
    assert p.kernel == kernel_of(D, pfft_form) and p.decim == D and p.hist_len == heq.size - 1
    assert launch_shape(n_out, V, D, n_cu_of(torch_cuda))[0] == frames
    y, _ = run_pfft(torch_cuda, p, np.array(x), n_out, hist=np.array(hist), want_hist=False)  # the case's arrays are read-only
    acc.gate("A %s %s Q=%d frames=%d" % (name, p.kernel, Q, frames), y, model, r, frames)


@gpu
@pytest.mark.parametrize("name", ["c5", "d8-L2049"])
def test_layout_b(torch_cuda, name, pfft_form):
    """Position = (k, q): eight frames in every workgroup, every workgroup full."""
    n_cu = n_cu_of(torch_cuda)
    D = geometry(CHAINS[name])[1]
    max_wg = n_cu * (1 if D == 16 else 2)
    stages, heq, D, Q, V, n_out, x, hist, r, model = case_b(name, max_wg)
    nf, fpw, wgs = launch_shape(n_out, V, D, n_cu)
    assert fpw == FPW and nf == FPW * wgs and wgs == max_wg
    p = nsh.FirCascadePlan(stages)
    assert p.kernel == kernel_of(D, pfft_form)
    y, _ = run_pfft(torch_cuda, p, np.array(x), n_out, hist=np.array(hist), want_hist=False)  # the case's arrays are read-only
    (yb, frames), (mb, _), (rb, _) = by_workgroup(y, FPW, V), by_workgroup(model, FPW, V), by_workgroup(r, FPW, V)
    assert frames == wgs
    acc.gate("B %s %s Q=%d workgroups=%d" % (name, p.kernel, Q, wgs), yb, mb, rb, frames)


# ---- the per-frame scale is exact -----------------------------------------------------------------------
SCALE_EXPONENTS = (60, -60, 125, -110)  # the scale arm, and form 2's pass-1 re-do arm, on both sides
FP32_MAX = float(np.finfo(np.float32).max)
FP32_TINY = float(np.finfo(np.float32).tiny)


def scale_input(D, n_out):
    """Multiples of 2^-10 with |re|, |im| <= 2: exact in fp32 at every exponent used."""
    x0 = int_signal(np.random.default_rng(17), D * n_out) * np.float32(0.25)
    assert np.all(x0.view(np.float32) * 1024 == np.round(x0.view(np.float32) * 1024)) and np.abs(x0.view(np.float32)).max() == 2.0
    return x0


def fits_fp32(x0, stages, e):
    """The contract's ceiling of an output of x0 2^e, max|x| sum|heq|, lies inside fp32."""
    return float(np.abs(x0).max()) * 2.0 ** e * heq_l1(stages) < 3.0e38


def scaled_outputs(y0, e):
    """ldexp(y0, e) per fp32 component, and which components the assertion covers: y0 zero, or
    y0 2^e a normal fp32 number."""
    c = y0.view(np.float32).astype(np.float64)
    want = np.ldexp(c, e)
    ok = (c == 0.0) | ((np.abs(want) >= FP32_TINY) & (np.abs(want) <= FP32_MAX))
    return np.where(ok, want, 0.0).astype(np.float32), ok


@pytest.mark.parametrize("name", ["c5", "d16-L4097", "d8-L2049"])
def test_cpu_scale_cases_cover_their_outputs(name):
    """On the model's outputs: the share that test_scale_is_exact's condition leaves out (under 1 %), and
    that every exponent fits fp32 (C5 at 125 too: max|x0| 2^125 sum|heq| < 3e38)."""
    stages = CHAINS_B[name]
    heq, D, Q, V = geometry(stages)
    n_out = 64 * V + 1
    x0 = scale_input(D, n_out)
    y0 = pfft_model(x0, None, stages, n_out)
    for e in SCALE_EXPONENTS:
        assert fits_fp32(x0, stages, e)
        _, ok = scaled_outputs(y0, e)
        print("SCALE %s e=%d: %.4f %% of the outputs left out" % (name, e, 100.0 * (1.0 - ok.mean())))
        assert 1.0 - ok.mean() < 0.01


@gpu
@pytest.mark.parametrize("name", ["c5", "d16-L4097", "d8-L2049"])
def test_scale_is_exact(torch_cuda, name, pfft_form):
    """The per-frame power-of-two scale changes no output bit: three or four frames per workgroup, x0 in
    multiples of 2^-10 with |x0| <= 2 (its frames are not scaled), and x0 2^e for e = 60, -60 (scaled) and
    125, -110 (form 2 redoes pass 1 on scaled rows): the outputs are ldexp(y(x0), e) bit for bit, wherever
    that is zero or a normal number."""
    n_cu = n_cu_of(torch_cuda)
    stages = CHAINS_B[name]
    heq, D, Q, V = geometry(stages)
    n_out = many_frames_n_out(V, D, n_cu)
    assert launch_shape(n_out, V, D, n_cu)[1] >= 3
    x0 = scale_input(D, n_out)
    p = nsh.FirCascadePlan(stages)
    assert p.kernel == kernel_of(D, pfft_form)
    y0, _ = run_pfft(torch_cuda, p, x0, n_out, want_hist=False)
    assert np.all(np.isfinite(y0.view(np.float32))) and np.any(y0 != 0)
    for e in SCALE_EXPONENTS:
        assert fits_fp32(x0, stages, e)  # C5 at 125 too
        x = (x0.astype(np.complex128) * 2.0 ** e).astype(np.complex64)
        assert np.all(x.astype(np.complex128) == x0.astype(np.complex128) * 2.0 ** e)
        y, _ = run_pfft(torch_cuda, p, x, n_out, want_hist=False)
        want, ok = scaled_outputs(y0, e)
        left_out = 1.0 - ok.mean()
        print("SCALE %s %s e=%d: %.4f %% of the outputs left out" % (name, p.kernel, e, 100.0 * left_out))
        assert left_out < 0.01
        got = np.where(ok, y.view(np.float32), np.float32(0.0))
        assert np.array_equal(bits(got), bits(want)), (name, e, first_mismatch(bits(got), bits(want)))
