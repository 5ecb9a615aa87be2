"""The accuracy gate of the time-domain kernels: fir_filter_ccf in all its forms (k_fir_direct,
k_fir_f32mfma, k_fir_mfma12 / 13 / 11), freq_xlating_fir_filter_ccf (k_fir_xlat), rotator_cc
(k_rotate), rational_resampler_ccf (k_resamp), pfb_arb_resampler_ccf (k_arb), pfb_channelizer_ccf
(k_pfb) and pfb_synthesizer_ccf (k_pfb_synth), each held to the rms error, over the whole call and at
its worst position, of an fp32 model that sums in the order the kernel's header documents
(tests/fir_accuracy.py: models, references, positions, and the factors with the figures they come from).

Every other float-data test of these kernels ends in oracle.tol_ok at 1e-5, which a correct fp32
kernel meets five to twenty-eight times over: a tap image off in its low bits, a phasor or a mu
short of bits, a dropped low term of the fp16x2 split all pass it, and integer data (exact in any
order) cannot show them. Here they do not pass (the CPU tests below, not marked gpu, prove it per
family on the models themselves), except the ones listed in fir_accuracy.py as not visible.

Part 3 (test_*split_alone*): one and two taps through FirPlan(MFMA), where the split is the only
error, against the per-element bound of nsh_fir_mfma_shared.hpp's own statement (fir_accuracy.split_bound).

nsh_fir_cascade_ccf (overlap-save on the composite filter) has the same gate against a complex64 model
of its chain in tests/test_gpu_pfft_accuracy.py.
k_pfb<64> and k_pfb_synth<64> take at most 1024 taps (16 per branch), so their case is L = 1024, not 32 M.
Neither FirPlan nor the library tells a caller which chunks went to the exact forms; the split-alone
cases assert plan.kernel and restate chunk_needs_exact on the inputs (no chunk qualifies).

Measured on one MI355X (profiles/fir_accuracy_ratios.log; kernel error and kernel / model, the models'
errors being the kernels' wherever the ratio is 1.000; every case passes, no kernel needed a change and
no model an extension):
                                         whole                        worst position
  k_fir_direct D = 1, 2, 4, 8, L = 127   1.80e-7..1.91e-7  1.000      2.44e-7..2.88e-7  1.000
  k_fir_direct<1,8> L = 3617             9.54e-7           1.000      1.42e-6           1.000
  k_fir_f32mfma<9>, <17>                 1.81e-7, 2.56e-7  1.000      2.69e-7, 3.75e-7  1.000
  k_fir_mfma12<1> L = 1                  5.42e-8           1.000      7.13e-8           1.000
  k_fir_mfma12<6> L = 161                1.02e-7           0.796      1.45e-7           0.796
  k_fir_mfma13 / 11<2,5> L = 127         9.09e-8           0.828      1.25e-7           0.829
  k_fir_mfma13 / 11<4,3> L = 127         9.93e-8           0.865      1.22e-7           0.913
  k_fir_xlat untuned, 6 cases            1.11e-7..2.90e-7  1.000      1.18e-7..3.16e-7  1.000
  k_fir_xlat at 0.1137, 6 cases          1.26e-7..2.95e-7  1.000..1.003  1.38e-7..3.23e-7  0.995..1.019
  k_rotate, 2 cases                      5.94e-8           1.001..1.009  7.70e-8..8.31e-8  1.003..1.012
  k_resamp, 4 cases                      7.29e-8..5.17e-7  1.000      1.03e-7..7.60e-7  1.000
  k_arb, 4 cases (and k_resamp's model)  6.39e-8..5.69e-7  1.000      9.46e-8..8.46e-7  1.000
  k_pfb<2>, <32>, <64>                   9.61e-8..1.27e-7  1.000      1.36e-7..1.79e-7  1.000
  k_pfb_synth<2>, <32>, <64>             9.67e-8..1.28e-7  1.000      1.53e-7..1.85e-7  1.000
  the split alone, 15 cases              worst error / bound 0.369..0.415 (the 16-term model 0.369..0.391)
The fp16x2 rows are against the 4-term grouping, which they are gated by. The hardware sits on neither of
the two groupings the gate was set up with: against groups of 16 the ratios are 1.223 / 1.285 (mfma12<6>),
1.176 / 1.225 (<2,5>) and 1.115 / 1.146 (<4,3>). It sits on exact groups of 8, the eight k one lane holds
of a v_mfma_f32_32x32x16_f16 or 16x16x32 operand: 1.011 / 1.022, 1.021 / 0.972 and 1.011 / 1.015, with 72 %,
60 % and 58 % of the outputs equal to that model bit for bit (12 to 19 % for groups of 16, 6 to 12 % for
groups of 4); what is left is the order in which an MFMA adds its two or four groups of 8 to the
accumulator, which the model takes ascending. With one tap all groupings are one product and the
kernel equals them bit for bit. The two walks give the same figures as each other in every case here.
The tuned k_fir_xlat and k_rotate differ from their models by the device's sincospif against a correctly
rounded cos / sin."""
import numpy as np
import pytest

from tests import fir_accuracy as acc
from tests.fft_xlat_ref import phase_inc
from tests.gpu_util import dev, uniform

gpu = pytest.mark.gpu

FREQ = 0.1137
FIRST = 12345


def lowpass(L, cutoff, seed, gain=1.0):
    """Hamming-windowed sinc at `cutoff` cycles per sample, every tap times a seeded factor in [0.9, 1.1]:
    no symmetry for a kernel to lean on."""
    k = np.arange(L) - (L - 1) / 2.0
    r = np.random.default_rng(seed)
    return (gain * 2 * cutoff * np.sinc(2 * cutoff * k) * np.hamming(L) * r.uniform(0.9, 1.1, L)).astype(np.float32)


def tap_off(h, k=None):
    """One dominant tap (the largest unless given) times 1 + 1e-6."""
    g = h.copy()
    k = int(np.argmax(np.abs(h))) if k is None else k
    g[k] = np.float32(np.float64(g[k]) * (1.0 + 1e-6))
    assert g[k] != h[k]
    return g


def table_off(M):
    """k_pfb's tables with one entry of the first stage times 1 + 1e-6."""
    t = [(a.copy(), b.copy()) for a, b in acc.pfb_tables(M)]
    lane = M // 2 + 1
    for part in t[0]:
        part[lane] = np.float32(part[lane] * (1.0 + 1e-6))
    return t


# ---- CPU: per family, what the gate lets through and what it does not ----------------------------------
def _fir_family():
    D, L, n = 4, 127, 64 * 1024
    h, x, hist = lowpass(L, 0.1, 1), uniform(n * D, 2), uniform(L - 1, 3)
    m = lambda **kw: acc.fir_model(x, hist, kw.pop("taps", h), D, n, **kw)
    half = list(range(0, L, 2)) + list(range(1, L, 2))
    return dict(frames=64, r=acc.fir_ref(x, hist, h, D, n), model=m(),
                correct={"product rounded, then added": m(fma=False)},
                defects={"centre tap x (1 + 1e-6)": m(taps=tap_off(h)),
                         "order: k descending": m(order=range(L - 1, -1, -1)),
                         "order: even taps, then odd taps": m(order=half)})


def _f32mfma_family():
    L, n = 127, 64 * 2048
    h, x, hist = lowpass(L, 0.1, 4), uniform(n, 5), uniform(L - 1, 6)
    m = lambda **kw: acc.f32mfma_model(x, hist, kw.pop("taps", h), n, **kw)
    return dict(frames=64, r=acc.fir_ref(x, hist, h, 1, n), model=m(),
                correct={"product rounded, then added": m(fma=False)},
                defects={"centre tap x (1 + 1e-6)": m(taps=tap_off(h))})


def _split_family(D):
    L, F = 127, acc.frames_for(2048 // D)
    n = F * (2048 // D)
    h, x, hist = lowpass(L, 0.4 / D, 7 + D), uniform(n * D, 8 + D), uniform(L - 1, 9 + D)
    f = acc.mfma12_model if D == 1 else (lambda *a, **kw: acc.decim_model(a[0], a[1], a[2], D, *a[3:], **kw))
    m = lambda group, **kw: f(x, hist, kw.pop("taps", h), n, group, **kw)
    return dict(frames=F, r=acc.fir_ref(x, hist, h, D, n), model=m(4),
                correct={"groups of 16 terms": m(16), "groups of 8 terms (where the hardware was found)": m(8)},
                defects={"centre tap x (1 + 1e-6), groups of 16": m(16, taps=tap_off(h)),
                         "centre tap x (1 + 1e-6), groups of 4": m(4, taps=tap_off(h)),
                         "taps' low fp16 term dropped": m(16, drop_lo=True),
                         "split truncates, groups of 16": m(16, trunc=True),
                         "split's low terms truncate, groups of 16": m(16, trunc="lo")})


def _xlat_family():
    D, L, n = 16, 127, 128 * 512
    inc = phase_inc(-FREQ)
    h, x, hist = lowpass(L, 0.4 / D, 10), uniform(n * D, 11), uniform(L - 1, 12)
    m = lambda **kw: acc.xlat_model(x, hist, kw.pop("taps", h), D, inc, FIRST, n, **kw)
    return dict(frames=128, r=acc.xlat_ref_at(x, hist, h, D, inc, FIRST, n), model=m(),
                correct={"every sample's own phasor, rounded once": m(pair=False),
                         "products rounded, then added": m(fma=False)},
                defects={"centre tap x (1 + 1e-6)": m(taps=tap_off(h)),
                         "phasor from the top 24 phase bits": m(bits=24)})


def _rotate_family():
    n = 64 * 1024
    inc = phase_inc(FREQ)
    x = uniform(n, 13)
    m = lambda **kw: acc.rotate_model(x, inc, FIRST, **kw)
    return dict(frames=64, r=acc.rotate_ref(x, inc, FIRST), model=m(),
                correct={"every sample's own phasor, rounded once": m(pair=False),
                         "products rounded, then added": m(fma=False)},
                defects={"phasor from the top 24 phase bits": m(bits=24)})


def _resamp_family():
    I, D, L, units = 3, 2, 127, 64 * 680
    h, x, hist = lowpass(L, 0.4 / I, 14, gain=I), uniform(units * D, 15), uniform(acc.ceil_div(L, I) - 1, 16)
    m = lambda **kw: acc.resamp_model(x, hist, kw.pop("taps", h), I, D, units, **kw)
    return dict(frames=64, r=acc.resamp_ref(x, hist, h, I, D, units), model=m(),
                correct={"product rounded, then added": m(fma=False)},
                defects={"centre tap x (1 + 1e-6)": m(taps=tap_off(h))})


def _arb_family():
    F, L, n = 32, 384, 64 * 1024
    step, phase = int(round(F / (44.1 / 48) * 2 ** 32)), (4 << 32) + 0x89abcdef
    h, hist = lowpass(L, 0.4 / F, 17, gain=F), uniform(L // F - 1, 18)
    x = uniform(int(acc.arb_indices(step, F, phase, n)[0].max()) + 1, 19)
    m = lambda **kw: acc.arb_model(x, hist, kw.pop("taps", h), F, step, phase, n, **kw)
    # the planted tap is its own defect: the reference keeps d of the true taps, the model's d moves with it
    return dict(frames=64, r=acc.arb_ref(x, hist, h, F, step, phase, n), model=m(),
                correct={"products rounded, then added": m(fma=False)},
                defects={"centre tap x (1 + 1e-6)": m(taps=tap_off(h)),
                         "mu from the top 16 fraction bits": m(mu_bits=16)})


def _pfb_family(synth):
    M, L, items = 32, 1024, 64 * 64
    h, x = lowpass(L, 0.4 / M, 20), uniform(items * M, 21)
    if synth:
        hist = uniform((L // M - 1) * M, 22)
        m = lambda **kw: acc.synth_model(x, hist, kw.pop("taps", h), M, **kw)
        r = acc.synth_ref(x, hist, h, M)
    else:
        hist = uniform(L - 1, 22)
        m = lambda **kw: acc.pfb_model(x, hist, kw.pop("taps", h), M, items, **kw).ravel()
        r = acc.pfb_ref(x, hist, h, M, items).ravel()
    return dict(frames=64, r=r, model=m(),
                correct={"products rounded, then added": m(fma=False)},
                defects={"centre tap x (1 + 1e-6)": m(taps=tap_off(h)),
                         "one DFT table entry x (1 + 1e-6)": m(tables=table_off(M))})


FAMILIES = {"k_fir_direct": _fir_family, "k_fir_f32mfma": _f32mfma_family,
            "k_fir_mfma12": lambda: _split_family(1), "k_fir_mfma13<2>": lambda: _split_family(2),
            "k_fir_mfma13<4>": lambda: _split_family(4), "k_fir_xlat": _xlat_family, "k_rotate": _rotate_family,
            "k_resamp": _resamp_family, "k_arb": _arb_family, "k_pfb": lambda: _pfb_family(False),
            "k_pfb_synth": lambda: _pfb_family(True)}
# defects that sit inside the spread of the correct implementations: fir_accuracy.py lists them too
NOT_VISIBLE = {("k_fir_direct", "order: k descending"), ("k_fir_direct", "order: even taps, then odd taps"),
               ("k_fir_mfma12", "split's low terms truncate, groups of 16"),
               ("k_fir_mfma13<2>", "split's low terms truncate, groups of 16"),
               ("k_fir_mfma13<4>", "split's low terms truncate, groups of 16")}
_families = {}


def family(name):
    if name not in _families:
        _families[name] = FAMILIES[name]()
    return _families[name]


@pytest.mark.parametrize("name", list(FAMILIES))
def test_cpu_correct_implementations_pass(name):
    """(a) A second correct implementation of the same order passes against the family's model."""
    c = family(name)
    for what, y in c["correct"].items():
        w, p = acc.ratios(y, c["model"], c["r"], c["frames"])
        print("SPREAD %s: %s: whole %.3f worst %.3f" % (name, what, w, p))
        acc.gate("%s model, %s" % (name, what), y, c["model"], c["r"], c["frames"])


@pytest.mark.parametrize("name", list(FAMILIES))
def test_cpu_defects_fail(name):
    """(b) Every planted defect fails at least one of the two gates, or is listed as not visible -- and
    then does pass, so the list stays true."""
    c = family(name)
    for what, y in c["defects"].items():
        w, p = acc.ratios(y, c["model"], c["r"], c["frames"])
        hidden = (name, what) in NOT_VISIBLE
        print("DEFECT %s: %s: whole %.3f worst %.3f%s" % (name, what, w, p, " (not visible to this gate)" if hidden else ""))
        if hidden:
            acc.gate("%s model, %s" % (name, what), y, c["model"], c["r"], c["frames"])
        else:
            with pytest.raises(AssertionError, match="whole|worst position"):
                acc.gate("%s model, %s" % (name, what), y, c["model"], c["r"], c["frames"])


def test_cpu_decimated_reference_is_xlat_ref():
    """xlat_ref_at (and fir_ref, rotate_ref) against xlat_ref's full-rate convolution."""
    inc = phase_inc(-FREQ)
    for D, L in ((1, 33), (5, 127), (64, 1024)):
        h, x, hist = lowpass(L, 0.4 / D, L), uniform(300 * D, D), uniform(L - 1, L + D)
        for i, f in ((0, 0), (inc, FIRST), (inc, 2 ** 64 - 1000)):
            a, b = acc.xlat_ref_at(x, hist, h, D, i, f, 300), acc.xlat_ref(x, hist, h, D, i, f, 300)
            assert np.max(np.abs(a - b)) <= 1e-13 * np.max(np.abs(b)), (D, L, i, f)
    x = uniform(500, 3)
    np.testing.assert_allclose(acc.rotate_ref(x, inc, FIRST), acc.xlat_ref(x, x[:0], np.ones(1, np.float32), 1, inc, FIRST, 500),
                               rtol=1e-15)


def _pfb_pair(M, L):
    h, x, H = uniform(L, 3 * L + M).real.copy(), uniform(40 * M, M), L - 1
    return H, x, lambda hist: (acc.pfb_ref_conv(x, hist, h, M, 40), acc.pfb_ref(x, hist, h, M, 40))


def _resamp_pair(I, D, L):
    h, x, H = uniform(L, 5 * L + I).real.copy(), uniform(50 * D, I + D), acc.ceil_div(L, I) - 1
    return H, x, lambda hist: (acc.resamp_ref_conv(x, hist, h, I, D, 50), acc.resamp_ref(x, hist, h, I, D, 50))


def _xlat_pair(D, L):
    h, x, H = uniform(L, 7 * L + D).real.copy(), uniform(30 * D, D), L - 1
    inc, first = 0x1234567890abcdef, 2 ** 40 + 7
    return H, x, lambda hist: (acc.xlat_ref_at(x, hist, h, D, inc, first, 30), acc.xlat_ref(x, hist, h, D, inc, first, 30))


REFERENCE_PAIRS = [(_pfb_pair, c) for c in ((2, 5), (8, 127), (64, 1024))] + \
                  [(_resamp_pair, c) for c in ((3, 2, 31), (1, 1, 1), (64, 7, 1024), (5, 64, 127))] + \
                  [(_xlat_pair, c) for c in ((1, 127), (5, 33), (64, 1024))]


@pytest.mark.parametrize("pair,case", REFERENCE_PAIRS,
                         ids=["%s-%s" % (p.__name__[1:-5], "-".join(map(str, c))) for p, c in REFERENCE_PAIRS])
def test_cpu_references_agree(pair, case):
    """The two float64 derivations of one block's reference (np.convolve from the definition against
    the polyphase sum; xlat_ref_at against xlat_ref) on a random history of full length, on hist=None
    and on an explicit zero history: max|a - b| <= 1e-12 max|b|. The 1e-12 is float64's 1.1e-16 times
    the 1024 terms of the longest sum, with a tenfold margin (the pairs stay below 1e-15 here);
    an indexing defect in either form gives O(1)."""
    H, x, both = pair(*case)
    for what, hist in (("random", uniform(max(H, 1), 99 + H)[:H]), ("none", None), ("zeros", np.zeros(H, np.complex64))):
        a, b = both(hist)
        worst = np.max(np.abs(a - b)) / np.max(np.abs(b))
        print("%s %s hist=%s: %.3g" % (pair.__name__, case, what, worst))
        assert a.shape == b.shape and worst <= 1e-12, (case, what, worst)
    for got, want in zip(both(None), both(np.zeros(H, np.complex64))):      # hist=None is a zero history, in each form
        np.testing.assert_array_equal(got, want)


def test_cpu_arb_model_without_mu_is_the_resampler_model():
    """(32, 32/21, 384) from phase 0: step = 21 2^32, mu = 0, w = h exactly: k_resamp's sum at I = 32, D = 21."""
    F, L, n = 32, 384, 32 * 40
    step = int(round(F / (32 / 21) * 2 ** 32))
    assert step == 21 << 32
    h, hist, x = lowpass(L, 0.4 / F, 1, gain=F), uniform(L // F - 1, 2), uniform(21 * 40 + 1, 3)
    np.testing.assert_array_equal(acc.arb_model(x, hist, h, F, step, 0, n), acc.resamp_model(x, hist, h, 32, 21, 40))


# ---- part 3 on the CPU: the models under the split's own bound ------------------------------------------
SPLIT_TAPS = {"1/3": [1.0 / 3.0], "0.7": [0.7], "pair 2^-12 apart": [0.7, 2.0 ** -11 / 3.0]}
SPLIT_CHUNKS = 16


# (defect, the model's switch, the tap sets at which it exceeds the bound). A truncating split is convicted
# at 0.7 and at the pair (1.01 to 1.10 of the bound) and not at 1/3, whose own split happens to lose
# little (0.73 to 0.75); a scale exponent one too low costs one bit of the smallest samples' low term
# and stays inside the bound everywhere (0.37 to 0.61, the model 0.37 to 0.39): the bound, which the
# model uses 0.39 of, has that much room.
SPLIT_DEFECTS = [("truncating split", dict(trunc=True), lambda taps: taps != "1/3"),
                 ("scale exponent + 1 (fp16 overflow)", dict(scale_off=1), lambda taps: True),
                 ("scale exponent - 1 (a bit lost)", dict(scale_off=-1), lambda taps: False),
                 ("unscale 2^+1", dict(unscale_off=1), lambda taps: True),
                 ("unscale 2^-1", dict(unscale_off=-1), lambda taps: True)]


def split_data(D, seed):
    """Seeded uniform 24-bit mantissas at exponents 0 .. -20 (every chunk holds both ends: 4096 draws),
    chunk c louder by 2^(c mod 3). One history sample for the two-tap filters."""
    r = np.random.default_rng(seed)
    n = SPLIT_CHUNKS * 2048 + 1

    def part():
        mant = (r.integers(1 << 23, 1 << 24, n).astype(np.float64)) * 2.0 ** -23
        return mant * 2.0 ** -r.integers(0, 21, n) * r.choice([-1.0, 1.0], n)

    v = (part() + 1j * part())
    v[9] = (2.0 - 2.0 ** -23) + 1j * (1.0 + 2.0 ** -23)      # the top of the range: one exponent more overflows fp16
    v[1:] *= np.repeat(2.0 ** (np.arange(SPLIT_CHUNKS) % 3), 2048)
    v = v.astype(np.complex64)
    assert np.all(v.astype(np.complex128) == v)
    return v[1:], v[:1]


def split_path_holds(x, hist, halo):
    """chunk_needs_exact restated: finite, and no nonzero component more than 2^28 below the largest
    magnitude of its chunk and halo (scaled below 2^-14)."""
    ext = np.concatenate([hist, x])
    mag = np.abs(np.stack([ext.real, ext.imag]).astype(np.float64))
    for c in range(x.size // 2048):
        w = mag[:, max(hist.size + 2048 * c - halo, 0):hist.size + 2048 * (c + 1)]
        if not np.all(np.isfinite(w)) or np.ldexp(w[w > 0].min(), acc.scale_exp(w.max())) < 2.0 ** -14:
            return False
    return True


def split_case(D, taps):
    h = np.asarray(SPLIT_TAPS[taps], np.float32)
    x, hist = split_data(D, 100 + D)
    hist = hist[:h.size - 1]
    n = x.size // D
    halo = 32 * ((h.size + 30) // 32) if D == 1 else D * 16 * (acc.decim_qh(h.size, D) - 1)
    ext = np.concatenate([hist, x])
    return h, x, hist, n, acc.fir_ref(x, hist, h, D, n), acc.split_bound(ext, h, D, n, halo), halo


def split_model(D, h, x, hist, n, group, **kw):
    if D == 1:
        return acc.mfma12_model(x, hist, h, n, group, **kw)
    return acc.decim_model(x, hist, h, D, n, group, **kw)


def bound_use(y, r, bound):
    e = np.stack([np.abs(y.real - r.real), np.abs(y.imag - r.imag)])
    return float(np.max(e / bound))


@pytest.mark.parametrize("taps", list(SPLIT_TAPS))
@pytest.mark.parametrize("D", [1, 2, 4])
def test_cpu_split_alone_models_meet_the_bound_and_defects_do_not(D, taps):
    """The part-1 models use at most half of the bound on the inputs of the GPU case. A sample scale
    one too high (fp16 overflow) and an unscale by the wrong power exceed it at every tap set, a
    truncating split at two of the three; SPLIT_DEFECTS says which do not and by how much."""
    h, x, hist, n, r, bound, halo = split_case(D, taps)
    assert split_path_holds(x, hist, halo)
    for group in (16, 4):
        use = bound_use(split_model(D, h, x, hist, n, group), r, bound)
        print("BOUND model D=%d taps %s groups of %d: worst error / bound %.3f" % (D, taps, group, use))
        assert use <= 0.5, (D, taps, group, use)
    model_use = use
    for what, kw, exceeds in SPLIT_DEFECTS:
        with np.errstate(invalid="ignore", over="ignore"):
            y = split_model(D, h, x, hist, n, 16, **kw)
            use = float("inf") if not np.all(np.isfinite(y)) else bound_use(y, r, bound)
        over = exceeds(taps)
        print("BOUND defect D=%d taps %s %s: worst error / bound %.3g%s" % (D, taps, what, use, "" if over else
                                                                           " (inside the bound: not convicted by it)"))
        assert use > 1.0 if over else model_use <= use <= 1.0, (D, taps, what, use)


def run_stream(torch, plan, x, hist, n_items, *args):
    """One call of a stream plan (x, hist_in, hist_out, y, n, ...): returns the n_items outputs."""
    dx = dev(torch, x)
    dh = dev(torch, hist) if hist.size else None
    dho = torch.zeros(max(hist.size, 1), dtype=torch.complex64, device="cuda")
    dy = torch.empty(n_items, dtype=torch.complex64, device="cuda")
    plan(dx, dh, dho, dy, *args)
    torch.cuda.synchronize()
    return dy.cpu().numpy()


def run_fir(torch, plan, x, hist, n_out):
    dx, dh = dev(torch, x), dev(torch, hist if hist.size else np.zeros(1, np.complex64))
    dho = torch.zeros_like(dh)
    dy = torch.empty(n_out, dtype=torch.complex64, device="cuda")
    plan(dx, dh, dho, dy, n_out)
    torch.cuda.synchronize()
    return dy.cpu().numpy()


def fir_case(torch, D, L, algo, kernel, positions, model, seed):
    from newsched_amd import nsh

    F = acc.frames_for(positions)
    n = F * positions
    h, x, hist = lowpass(L, 0.4 / D, seed), uniform(n * D, seed + 1), uniform(max(L - 1, 1), seed + 2)[:L - 1]
    plan = nsh.FirPlan(h, D, algo)
    assert plan.kernel == kernel, plan.kernel
    y = run_fir(torch, plan, x, hist, n)
    plan.close()
    r = acc.fir_ref(x, hist, h, D, n)
    return "%s L=%d frames=%d" % (plan.kernel, L, F), y, model(x, hist, h, n), r, F, (x, hist, h, n)


@gpu
@pytest.mark.parametrize("D,L", [(1, 127), (2, 127), (4, 127), (8, 127), (1, 3617)])
def test_fir_direct(torch_cuda, D, L):
    """k_fir_direct<D,R> at every decimation, and at 3617 taps (a window past 64 KiB of LDS)."""
    from newsched_amd import nsh
    name, y, model, r, F, _ = fir_case(torch_cuda, D, L, nsh.FIR_DIRECT, acc.direct_name(D), acc.positions_direct(D),
                                       lambda x, hist, h, n: acc.fir_model(x, hist, h, D, n), 1000 + L + D)
    acc.gate(name, y, model, r, F)


@gpu
@pytest.mark.parametrize("L", [127, 257])
def test_fir_f32mfma(torch_cuda, L):
    from newsched_amd import nsh
    name, y, model, r, F, _ = fir_case(torch_cuda, 1, L, nsh.FIR_MFMA_F32, "k_fir_f32mfma<%d>" % acc.qf(L), acc.positions_matrix(1),
                                       lambda x, hist, h, n: acc.f32mfma_model(x, hist, h, n), 2000 + L)
    acc.gate(name, y, model, r, F)


def split_gate(name, y, r, F, model, model4):
    """Gate against the 4-term grouping (the looser of the two the gate was set up with), print the ratio
    against groups of 16 and of 8 as well, and how many outputs equal the 8-term model bit for bit."""
    for group in (16, 8):
        m = model(group)
        w, p = acc.ratios(y, m, r, F)
        print("RATIO accuracy against groups of %d: whole ratio %.3f worst ratio %.3f bit-equal %.3f %s"
              % (group, w, p, float(np.mean(m.astype(np.complex64) == y)), name))
    acc.gate(name + " (groups of 4)", y, model4, r, F)


def mfma12_lengths():
    tops = {acc.q12(L): L for L in acc.ENDS_12}           # the last L of every bucket
    return [tops[min(tops)], tops[max(tops)]]


@gpu
@pytest.mark.parametrize("which", [0, 1], ids=["smallest bucket", "largest bucket"])
def test_fir_mfma12(torch_cuda, which):
    """k_fir_mfma12<Q> at the top of its smallest (one tap) and its largest (161 taps) bucket. The hardware
    sits on neither grouping the gate was set up with but between them, on groups of 8: see the table."""
    from newsched_amd import nsh
    L = mfma12_lengths()[which]
    name, y, m4, r, F, (x, hist, h, n) = fir_case(torch_cuda, 1, L, nsh.FIR_MFMA, "k_fir_mfma12<%d>" % acc.q12(L),
                                                  acc.positions_matrix(1),
                                                  lambda x, hist, h, n: acc.mfma12_model(x, hist, h, n, 4), 3000 + L)
    split_gate(name, y, r, F, lambda group: acc.mfma12_model(x, hist, h, n, group), m4)


@gpu
@pytest.mark.parametrize("walk,mask", [("k_fir_mfma13", "20"), ("k_fir_mfma11", "0")])
@pytest.mark.parametrize("D", [2, 4])
def test_fir_decimators(torch_cuda, monkeypatch, D, walk, mask):
    """k_fir_mfma13 and k_fir_mfma11 (NSH_DEC_WALK_MASK) at decim 2 and 4, 127 taps. The hardware sits
    between the two groupings, on groups of 8: see the table."""
    from newsched_amd import nsh

    monkeypatch.setenv("NSH_DEC_WALK_MASK", mask)
    L, pred = 127, walk == "k_fir_mfma11"
    name, y, m4, r, F, (x, hist, h, n) = fir_case(
        torch_cuda, D, L, nsh.FIR_MFMA, "%s<%d,%d>" % (walk, D, acc.decim_qh(L, D)), acc.positions_matrix(D),
        lambda x, hist, h, n: acc.decim_model(x, hist, h, D, n, 4, pred), 4000 + D)
    split_gate(name, y, r, F, lambda group: acc.decim_model(x, hist, h, D, n, group, pred), m4)


XLAT_CASES = [(4, 127), (8, 127), (16, 127), (32, 127), (64, 127), (64, 1024)]


@gpu
@pytest.mark.parametrize("freq", [0.0, FREQ], ids=["untuned", "tuned"])
@pytest.mark.parametrize("D,L", XLAT_CASES)
def test_fir_xlat(torch_cuda, D, L, freq):
    """One D per instantiation of k_fir_xlat<R,S>, and 1024 taps at D = 64 (four wave parts of 256 taps)."""
    from newsched_amd import nsh

    plan = nsh.FirXlatPlan(lowpass(L, 0.4 / D, 5000 + D + L), D, freq)
    assert plan.kernel == "k_fir_xlat<%d,%d>" % acc.xlat_form(D)[:2], plan.kernel
    assert (plan.inc == 0) == (freq == 0.0)
    F = acc.frames_for(plan.tile)
    n = F * plan.tile
    h, x, hist = lowpass(L, 0.4 / D, 5000 + D + L), uniform(n * D, 5001 + D), uniform(L - 1, 5002 + D)
    y = run_stream(torch_cuda, plan, x, hist, n, n, FIRST)
    acc.gate("%s D=%d L=%d freq=%g frames=%d" % (plan.kernel, D, L, freq, F), y,
             acc.xlat_model(x, hist, h, D, plan.inc, FIRST, n), acc.xlat_ref_at(x, hist, h, D, plan.inc, FIRST, n), F)
    plan.close()


@gpu
@pytest.mark.parametrize("first", [FIRST, 2 ** 64 - 1000], ids=["12345", "wraps"])
def test_rotate(torch_cuda, first):
    from newsched_amd import nsh

    torch = torch_cuda
    F = acc.frames_for(acc.POSITIONS_ROTATE)
    n = F * acc.POSITIONS_ROTATE
    inc = nsh.phase_inc(FREQ)
    x = uniform(n, 5500)
    dx = dev(torch, x)
    dy = torch.empty_like(dx)
    assert dx.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0      # the 16-byte path, pairs from sample 0
    nsh.rotate_cc(dx, dy, n, inc, first)
    torch.cuda.synchronize()
    acc.gate("k_rotate first_index=%d frames=%d" % (first, F), dy.cpu().numpy(), acc.rotate_model(x, inc, first),
             acc.rotate_ref(x, inc, first), F)


@gpu
@pytest.mark.parametrize("I,D,L", [(1, 1, 1024), (3, 2, 127), (7, 5, 255), (64, 63, 1024)])
def test_resamp(torch_cuda, I, D, L):
    from newsched_amd import nsh

    h = lowpass(L, 0.4 / max(I, D), 6000 + I + D, gain=I)
    plan = nsh.ResampPlan(h, I, D)
    F = acc.frames_for(plan.tile * I)
    units = F * plan.tile
    x, hist = uniform(units * D, 6001 + I), uniform(max(plan.history, 1), 6002 + I)[:plan.history]
    y = run_stream(torch_cuda, plan, x, hist, units * I, units)
    acc.gate("%s I=%d D=%d L=%d frames=%d" % (plan.kernel, I, D, L, F), y, acc.resamp_model(x, hist, h, I, D, units),
             acc.resamp_ref(x, hist, h, I, D, units), F)
    plan.close()


ARB_CASES = [(32, 44.1 / 48, 384, (4 << 32) + 0x89abcdef), (2, 1 / 1.37, 2048, (4 << 32) + 0x89abcdef),
             (64, 1.0 + 30e-6, 2048, (4 << 32) + 0x89abcdef), (32, 32 / 21, 384, 0)]


@gpu
@pytest.mark.parametrize("F,rate,L,phase", ARB_CASES, ids=["44.1/48", "1/1.37", "1+30e-6", "32/21"])
def test_arb(torch_cuda, F, rate, L, phase):
    """The last case starts at phase 0 with step = 21 2^32: mu = 0 in every output, and k_arb is gated
    against k_resamp's model at I = 32, D = 21 as well."""
    from newsched_amd import nsh

    torch = torch_cuda
    h = lowpass(L, 0.4 / F * min(1.0, rate), 7000 + F + L, gain=F)
    plan = nsh.ArbPlan(h, rate, F)
    frames = acc.frames_for(plan.tile)
    n = frames * plan.tile
    step = plan.step
    n_in = int(acc.arb_indices(step, F, phase, n)[0].max()) + 1
    assert plan.span(phase, n_in, n)[0] == n
    x, hist = uniform(n_in + 2, 7001 + F), uniform(max(plan.history, 1), 7002 + F)[:plan.history]
    dx, dh = dev(torch, x), dev(torch, hist) if hist.size else None
    dho = torch.zeros(max(hist.size, 1), dtype=torch.complex64, device="cuda")
    dy = torch.empty(n, dtype=torch.complex64, device="cuda")
    plan(dx, n_in, dh, dho, dy, n, phase)
    torch.cuda.synchronize()
    y = dy.cpu().numpy()
    name = "%s F=%d rate=%.9g L=%d frames=%d" % (plan.kernel, F, rate, L, frames)
    model, r = acc.arb_model(x, hist, h, F, step, phase, n), acc.arb_ref(x, hist, h, F, step, phase, n)
    acc.gate(name, y, model, r, frames)
    if phase == 0:
        assert step == 21 << 32 and n % 32 == 0
        units = n // 32
        np.testing.assert_array_equal(acc.resamp_model(x, hist, h, 32, 21, units), model)
        acc.gate(name + " (k_resamp's model)", y, acc.resamp_model(x, hist, h, 32, 21, units), r, frames)
    plan.close()


def pfb_taps(M):
    return min(32 * M, 1024)


@gpu
@pytest.mark.parametrize("M", [2, 32, 64])
def test_pfb(torch_cuda, M):
    from newsched_amd import nsh

    L = pfb_taps(M)
    h = lowpass(L, 0.4 / M, 8000 + M)
    plan = nsh.PfbPlan(h, M)
    F = acc.frames_for(plan.tile * M)
    items = F * plan.tile
    x, hist = uniform(items * M, 8001 + M), uniform(L - 1, 8002 + M)
    y = run_stream(torch_cuda, plan, x, hist, items * M, items)
    acc.gate("%s L=%d frames=%d" % (plan.kernel, L, F), y, acc.pfb_model(x, hist, h, M, items).ravel(),
             acc.pfb_ref(x, hist, h, M, items).ravel(), F)
    plan.close()


@gpu
@pytest.mark.parametrize("M", [2, 32, 64])
def test_pfb_synth(torch_cuda, M):
    from newsched_amd import nsh

    L = pfb_taps(M)
    h = lowpass(L, 0.4 / M, 9000 + M, gain=M)
    plan = nsh.PfbSynthPlan(h, M)
    F = acc.frames_for(plan.tile * M)
    items = F * plan.tile
    x, hist = uniform(items * M, 9001 + M), uniform((acc.ceil_div(L, M) - 1) * M, 9002 + M)
    y = run_stream(torch_cuda, plan, x, hist, items * M, items)
    acc.gate("%s L=%d frames=%d" % (plan.kernel, L, F), y, acc.synth_model(x, hist, h, M), acc.synth_ref(x, hist, h, M), F)
    plan.close()


# ---- GPU, part 3: the split with nothing else in the sum --------------------------------------------------
SPLIT_WALKS = [(1, "k_fir_mfma12", None), (2, "k_fir_mfma13", "20"), (4, "k_fir_mfma13", "20"), (2, "k_fir_mfma11", "0"),
               (4, "k_fir_mfma11", "0")]


@gpu
@pytest.mark.parametrize("taps", list(SPLIT_TAPS))
@pytest.mark.parametrize("D,walk,mask", SPLIT_WALKS)
def test_fir_split_alone_meets_its_bound(torch_cuda, monkeypatch, D, walk, mask, taps):
    """One tap: |y - x h| <= 4 2^-22 |x h| + 2^-38 max|chunk| max|h| per component, from the header's
    statement of the split alone; two taps: both terms' bounds and one more rounding. The split path
    runs: the plan names the split kernel and no chunk meets chunk_needs_exact's rule."""
    from newsched_amd import nsh

    if mask is not None:
        monkeypatch.setenv("NSH_DEC_WALK_MASK", mask)
    h, x, hist, n, r, bound, halo = split_case(D, taps)
    assert split_path_holds(x, hist, max(halo, 2048))
    plan = nsh.FirPlan(h, D, nsh.FIR_MFMA)
    assert plan.kernel.startswith(walk + "<"), plan.kernel
    y = run_fir(torch_cuda, plan, x, hist, n)
    plan.close()
    use = bound_use(y, r, bound)
    print("RATIO split alone %s taps %s: worst error / bound %.3f (model, groups of 16: %.3f)"
          % (plan.kernel, taps, use, bound_use(split_model(D, h, x, hist, n, 16, pred=walk == "k_fir_mfma11") if D > 1 else
                                                split_model(D, h, x, hist, n, 16), r, bound)))
    assert use <= 1.0, (plan.kernel, taps, use)
