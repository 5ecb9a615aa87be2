"""The LDS layouts that the plans of k_resamp and k_arb choose in C++
(newsched_amd/csrc/nsh_stream_layout.hpp, printed by tests/cpp/qa_stream_layout.cpp) against their
restatements in Python (CPU only). No output of a kernel depends on these choices, only its speed: a
chooser that went wrong after an edit would pass every parity test.

  * k_resamp: (R, G, a) for the 100 (I, D) pairs of tests/test_resamp_layout.py against its tile()
    and padding(), the model whose bank multiplicities that file asserts.
  * k_arb: (a, pad) for every (F, s) of the k_arb cases of tests/test_gpu_stream_forms.py (the steps
    on both sides of every change of instantiation; tests/fir_accuracy.py holds the list). It restates the dispatch, not the
    layout, so a and pad are restated here, from nsh_arb.hip's header: 32 consecutive outputs at
    sampled phases, the shift a of the sample image among 31 (none), 6 .. 1 for r < 1, the pad of the
    taps' upper half row among 0 .. 31 for F = 64, the first candidate with the smallest worst
    number of different entries on one bank pair.
"""
import numpy as np

from tests.test_cpp_runtime import run
from tests.fir_accuracy import arb_cases, arb_form
from tests.test_resamp_layout import PAIRS, linear, padding, tile


def lines(kind, cases):
    out = run("qa_stream_layout", 120, kind, *[str(v) for c in cases for v in c])
    rows = [[int(v) for v in l.split()[1:]] for l in out.splitlines() if l.startswith(kind + " ")]
    assert len(rows) == len(cases)
    return rows


def test_resamp_layout_is_the_models():
    got = lines("resamp", PAIRS)
    for (I, D), row in zip(PAIRS, got):
        R, G = tile(I, D)
        assert row == [I, D, R, int(linear(I, D)), G, padding(I, D)[0]], (I, D)
    assert {row[2] for row in got} == {1, 2, 4, 8} and {row[5] for row in got} >= {31, 4, 1}


def multiplicity(v):
    """worst number of different entries on one bank pair (entry mod 32) over the rows of v (groups of
    32 lanes): equal entries are a broadcast"""
    v = np.sort(v, axis=1)
    new = np.ones(v.shape, bool)
    new[:, 1:] = v[:, 1:] != v[:, :-1]
    on_bank = ((v[:, :, None] & 31) == np.arange(32)) & new[:, :, None]
    return int(on_bank.sum(axis=1).max())


def arb_positions(step, fshift):
    """pos of output l < 32 of a group that starts at c: whole inputs and whole filter steps, and
    quarters of a step on top"""
    ci, cf = np.meshgrid(np.arange(64, dtype=np.uint64), np.arange(4, dtype=np.uint64), indexing="ij")
    c = (ci << np.uint64(32 + fshift)) + (ci << np.uint64(32)) + (cf << np.uint64(30))
    return c.reshape(-1, 1) + np.arange(32, dtype=np.uint64)[None, :] * np.uint64(step)


def first_least(candidates, cost):
    costs = [cost(c) for c in candidates]
    return candidates[costs.index(min(costs))]


def arb_layout(F, s):
    fshift, step = F.bit_length() - 1, s << 27
    pos = arb_positions(step, fshift)
    linear_, a, pad = step <= F << 32, 31, 0
    if not linear_:
        smp = (pos >> np.uint64(32 + fshift)).astype(np.int64)
        a = first_least([31, 6, 5, 4, 3, 2, 1], lambda a: multiplicity(smp + (smp >> a)))
    if F == 64:
        j = ((pos >> np.uint64(32)) & np.uint64(63)).astype(np.int64)
        pad = first_least(list(range(32)), lambda pad: multiplicity(j + (j >> 5) * pad))
    return int(linear_), a, pad


def test_arb_layout_is_the_restatement():
    cases = sorted({(F, s) for F, L, s in arb_cases()})
    got = lines("arb", cases)
    for (F, s), row in zip(cases, got):
        assert row == [F, s, *arb_layout(F, s)], (F, s)
        assert all(bool(row[2]) == bool(arb_form(F, L, s)[1]) for L in (1, 2048))
    # both choices are exercised: padded and packed images, and tap rows with and without a pad
    assert {row[3] for row in got if not row[2]} >= {31, 6} and all(row[3] == 31 for row in got if row[2])
    assert {row[4] for row in got if row[0] != 64} == {0} and any(row[4] for row in got if row[0] == 64)
