"""GPU parity for nsh_fir_cascade_ccf (k_fir_pfft: a chain of decimating fir_filter_ccf stages
computed in one pass as the composite filter by polyphase-FFT overlap-save) against the oracle's
stage-by-stage chain (oracle.fir_ccf per stage, double accumulation, fp32 between stages):

* BASELINE config C5 (4 x fir(firwin(127, 0.45), 2)) at every frame-boundary shape: one output,
  partial frames, exactly one frame (V = 393), several workgroups, a ragged last frame;
* other chains with total decimation 16 and 8 (mixed tap lengths and decimations, single long
  stages), the reference-convention golden 4-stage chain (tests/golden/fir127_decim2.npz);
* call splitting through the (len(heq) - 1)-sample history, nonzero starting history;
* inf/NaN inputs (the chain's NaN and inf positions exactly: such frames run the staged chain),
  per-frame power-of-two scaling over 1e-30 .. 1e30 regions (checked against a +-512-output local
  envelope), a loud burst beside a quiet signal (the frame-relative accuracy contract),
  determinism.

Every test runs on both forms of the 16-phase kernel (NSH_PFFT_FORM at plan creation): 2 =
k_fir_pfft2<16> (round 5, the default: no LDS ring, pass 1 on the loaded rows, double-buffered
phase images) and 1 = k_fir_pfft<16,1> (the ring form); decimation-8 plans have one
form (k_fir_pfft<8,1>).

Tolerance: the north-star 1e-5 (oracle.tol_ok) on the final outputs."""
import numpy as np
import pytest

from oracle import oracle as orc
from newsched_amd import nsh
from tests.pfft_ref import C5, KERNEL16, _firwin, heq_l1, pfft_form, ref_chain, run_pfft  # noqa: F401  (pfft_form: autouse)

pytestmark = pytest.mark.gpu


def tol_pfft(y, r, x, stages, rel=1e-5):
    """oracle.tol_ok with the scale floored at 1e-2 of the input level max|x| sum|heq|: transform
    rounding is relative to the frame's input, so outputs far below it (the first outputs of a
    stream from zero history, where only the filter's tiny edge taps have data) carry an absolute
    error of ~1e-10 of the input level -- 1e-7 of that floor, against which 1e-5 is checked."""
    r = np.asarray(r, np.complex128)
    floor = 1e-2 * (float(np.abs(x).max()) if x.size else 0.0) * heq_l1(stages)
    scale = max(float(np.abs(r).max()) if r.size else 0.0, floor)
    err = np.abs(np.asarray(y, np.complex128) - r)
    maxerr = float(err.max()) if err.size else 0.0
    ok = maxerr <= rel * scale and bool(np.all(err <= rel * np.abs(r) + 0.1 * rel * scale))
    return ok, maxerr, scale


def test_c5_plan_shape(torch_cuda, pfft_form):
    p = nsh.FirCascadePlan(C5)
    assert p.decim == 16 and p.hist_len == 1890 and p.kernel == KERNEL16[pfft_form]


@pytest.mark.parametrize("n_out", [1, 2, 118, 119, 383, 384, 385, 392, 393, 394, 768, 769, 786, 787, 5000,
                                   384 * 256 + 1, 393 * 256, 393 * 256 + 1, 100_003, 1 << 20])
def test_c5_vs_oracle_chain(torch_cuda, n_out):
    p = nsh.FirCascadePlan(C5)
    x = orc.synth(16 * n_out, n_out % 977)
    y, hout = run_pfft(torch_cuda, p, x, n_out)
    ry = ref_chain(x, C5)
    ok, err, scale = orc.tol_ok(y, ry) if n_out >= 256 else tol_pfft(y, ry, x, C5)
    assert ok, (n_out, err, scale)
    # the next call's history: the last 1890 inputs (zeros before the stream), bit-exact
    full = np.concatenate([np.zeros(1890, np.complex64), x])
    np.testing.assert_array_equal(hout, full[-1890:])


def test_c5_golden_chain4(torch_cuda):
    """tests/golden/fir127_decim2.npz: y_chain4 = 4 x fir(taps, 2) of x (scipy lfilter-pinned)."""
    g = np.load("tests/golden/fir127_decim2.npz")
    taps, x, y4 = g["taps"], g["x"], g["y_chain4"]
    p = nsh.FirCascadePlan([(taps, 2)] * 4)
    y, _ = run_pfft(torch_cuda, p, x, x.size // 16)
    ok, err, scale = orc.tol_ok(y, y4)
    assert ok, (err, scale)


CHAINS = {
    "taps33-160-64-127": [(_firwin(33, 0.4), 2), (_firwin(160, 0.3), 2), (_firwin(64, 0.45), 2),
                          (_firwin(127, 0.45), 2)],
    "d4-d4": [(_firwin(255, 0.2), 4), (_firwin(127, 0.2), 4)],
    "d2-d8": [(_firwin(31, 0.45), 2), (_firwin(200, 0.1), 8)],
    "single-d16": [(_firwin(1501, 0.05), 16)],
    "single-d16-short": [(_firwin(7, 0.05), 16)],
    "single-d16-q188": [(_firwin(3000, 0.04), 16)],  # Q = 188: frames of 324 outputs
    "d2-d8-q129": [(_firwin(31, 0.45), 2), (_firwin(1011, 0.05), 8)],
    "d8-3x2": [(_firwin(127, 0.45), 2)] * 3,
    "single-d8": [(_firwin(900, 0.1), 8)],
    "d8-4x2": [(_firwin(127, 0.45), 2), (_firwin(61, 0.4), 4)],
}


@pytest.mark.parametrize("name", sorted(CHAINS))
@pytest.mark.parametrize("n_out", [1, 300, 4099, 200_001])
def test_chains_vs_oracle(torch_cuda, name, n_out):
    stages = CHAINS[name]
    p = nsh.FirCascadePlan(stages)
    assert p.decim == int(np.prod([d for _, d in stages]))
    x = orc.synth(p.decim * n_out, 31 + n_out)
    y, _ = run_pfft(torch_cuda, p, x, n_out)
    ry = ref_chain(x, stages)
    ok, err, scale = orc.tol_ok(y, ry) if n_out >= 256 else tol_pfft(y, ry, x, stages)
    assert ok, (name, n_out, err, scale)


def test_unsupported_chains_rejected(torch_cuda):
    with pytest.raises(nsh.NshError):
        nsh.FirCascadePlan([(_firwin(127, 0.45), 2)])            # D = 2
    with pytest.raises(nsh.NshError):
        nsh.FirCascadePlan([(_firwin(127, 0.45), 2)] * 5)        # D = 32
    with pytest.raises(nsh.NshError):
        nsh.FirCascadePlan([(_firwin(4200, 0.05), 16)])          # 263 overlap rows > 256
    with pytest.raises(nsh.NshError):
        nsh.FirCascadePlan([(np.array([1.0, np.inf], np.float32), 16)])


def test_c5_split_calls_and_history(torch_cuda):
    """Call-splitting invariance: calls shorter than a frame and than the history, ping-pong
    histories; equals the oracle chain over the whole stream."""
    p = nsh.FirCascadePlan(C5)
    n_total = 70_001
    x = orc.synth(16 * n_total, 5)
    ry = ref_chain(x, C5)
    cuts = [0, 1, 2, 50, 118, 119, 500, 893, 20_000, 20_001, n_total]
    hist = None
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        y, hist = run_pfft(torch_cuda, p, x[16 * a:16 * b], b - a, hist)
        parts.append(y)
    ok, err, scale = orc.tol_ok(np.concatenate(parts), ry)
    assert ok, (err, scale)


def test_c5_nonzero_start_history(torch_cuda):
    """A plan started from hist_in = the 1890 samples before x equals the chain over the longer
    stream (the composite state is the input history)."""
    p = nsh.FirCascadePlan(C5)
    pre, n_out = 16 * 200, 3000
    s = orc.synth(pre + 16 * n_out, 99)
    ry = ref_chain(s, C5)[pre // 16:]
    y, _ = run_pfft(torch_cuda, p, s[pre:], n_out, hist=s[pre - 1890:pre])
    ok, err, scale = orc.tol_ok(y, ry)
    assert ok, (err, scale)


def test_c5_deterministic(torch_cuda):
    p = nsh.FirCascadePlan(C5)
    n_out = 300_000
    x = orc.synth(16 * n_out, 3)
    y1, _ = run_pfft(torch_cuda, p, x, n_out)
    y2, _ = run_pfft(torch_cuda, p, x, n_out)
    np.testing.assert_array_equal(y1, y2)


@pytest.mark.parametrize("kind", ["nan", "inf", "neginf", "huge", "mixed"])
def test_c5_nonfinite_inputs(torch_cuda, kind):
    """Frames holding inf/NaN are computed by the staged chain itself (fp32 direct form, stage by
    stage over the frame's window): the NaN and the inf positions (re and im separately) are the
    chain's exactly -- 'mixed' puts +inf and -inf a few samples apart, so the chain's intermediate
    stages form inf - inf = NaN where the composite filter would give +-inf -- and every finite
    output is within tolerance. 'huge' (3e38, finite) must stay finite wherever the chain's output
    is (scaled transforms never overflow)."""
    p = nsh.FirCascadePlan(C5)
    n_out = 20_000
    x = orc.synth(16 * n_out, 7)
    val = {"nan": np.nan, "inf": np.inf, "neginf": -np.inf, "huge": 3.0e38, "mixed": np.inf}[kind]
    for pos in (0, 5000, 5001, 16 * 393 * 7 + 3, 16 * n_out - 1):
        x[pos] = complex(val, 0.25) if kind != "huge" else complex(val, -val)
        if kind == "mixed" and pos + 5 < x.size:
            x[pos + 5] = complex(-np.inf, -np.inf)
    y, _ = run_pfft(torch_cuda, p, x, n_out)
    ry = ref_chain(x, C5)
    for part in ("real", "imag"):
        a, b = getattr(y, part), getattr(ry, part)
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg="NaN positions (%s)" % part)
        np.testing.assert_array_equal(np.isinf(a), np.isinf(b), err_msg="inf positions (%s)" % part)
        np.testing.assert_array_equal(np.sign(a[np.isinf(b)]), np.sign(b[np.isinf(b)]), err_msg="inf signs (%s)" % part)
    if kind != "huge":
        assert not np.all(np.isfinite(ry)), "the case must exercise the non-finite path"
    fin = np.isfinite(ry.real) & np.isfinite(ry.imag)
    ok, err, scale = orc.tol_ok(y[fin], ry[fin])
    assert ok, (kind, err, scale)


@pytest.mark.parametrize("name", ["d8_three_stages", "d16_long_first"])
def test_chains_nonfinite_exact_pattern(torch_cuda, name):
    """The staged non-finite path on other chains (total decimation 8 and 16, mixed lengths)."""
    stages = {"d8_three_stages": [(_firwin(31, 0.4), 2), (_firwin(63, 0.45), 2), (_firwin(47, 0.4), 2)],
              "d16_long_first": [(_firwin(255, 0.2), 4), (_firwin(63, 0.4), 2), (_firwin(31, 0.45), 2)]}[name]
    p = nsh.FirCascadePlan(stages)
    D = p.decim
    n_out = 6000
    x = orc.synth(D * n_out, 3)
    for pos in (17, 4000, 4003, D * n_out // 2):
        x[pos] = complex(np.inf, np.nan if pos == 4003 else 1.0)
    x[4010] = complex(-np.inf, 0.5)
    y, _ = run_pfft(torch_cuda, p, x, n_out)
    ry = ref_chain(x, stages)
    for part in ("real", "imag"):
        a, b = getattr(y, part), getattr(ry, part)
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
        np.testing.assert_array_equal(np.isinf(a), np.isinf(b))
    fin = np.isfinite(ry.real) & np.isfinite(ry.imag)
    ok, err, scale = tol_pfft(y[fin], ry[fin], x[np.isfinite(x)], stages)
    assert ok, (name, err, scale)


def test_c5_mixed_amplitude_frame_relative_bound(torch_cuda):
    """transform rounding is relative to each frame's input level, not to each output.
    A 1e4 burst beside a 1e-3 signal: every output satisfies the frame-relative contract
    |y - r| <= 1e-5 |r| + 1e-6 max|x over its frame's window| sum|heq| (nsh_hip.h); the
    outputs of frames whose window holds no burst keep the per-sample 1e-5 bound; and the quiet
    outputs that share a frame with the burst are NOT held to 1e-5 of their own size (measured and
    asserted loosely, to document the contract rather than hide it)."""
    p = nsh.FirCascadePlan(C5)
    V, Q, D = 512 - 119, 119, 16
    n_out = 12 * V
    x = orc.synth(D * n_out, 5) * np.float32(1e-3)
    burst = slice(D * (5 * V) + 3000, D * (5 * V) + 3200)  # inside frame 5's new rows
    x[burst] *= np.float32(1e7)
    y, _ = run_pfft(torch_cuda, p, x, n_out)
    ry = ref_chain(x, C5)
    l1 = heq_l1(C5)
    ax = np.abs(x)
    err = np.abs(y.astype(np.complex128) - ry)
    lev = np.empty(n_out)
    for f in range((n_out + V - 1) // V):
        lo = max(0, D * (f * V - Q))
        lev[f * V:(f + 1) * V] = ax[lo:D * (f * V - Q) + D * 512].max()
    assert np.all(err <= 1e-5 * np.abs(ry) + 1e-6 * lev * l1), float((err / (1e-5 * np.abs(ry) + 1e-6 * lev * l1)).max())
    quiet = lev < 1.0  # frames whose window holds no burst
    assert quiet.sum() > 6 * V
    ok, e, sc = orc.tol_ok(y[quiet], ry[quiet])
    assert ok, (e, sc)
    worst = float((err[~quiet] / np.maximum(np.abs(ry[~quiet]), 1e-30)).max())
    assert worst > 1e-5  # documented: quiet outputs beside a burst are frame-relative, not per-sample


def _local_ok(y, r, half=512, rel=1e-5):
    """|y - r| <= rel |r| + 0.1 rel max|r| over the +-half outputs around each one."""
    from numpy.lib.stride_tricks import sliding_window_view as swv

    a = np.abs(np.asarray(r, np.complex128))
    env = swv(np.pad(a, half), 2 * half + 1).max(axis=1)
    err = np.abs(np.asarray(y, np.complex128) - r)
    bad = err > rel * a + 0.1 * rel * env
    return not bad.any(), int(bad.sum())


def test_c5_per_frame_scaling(torch_cuda):
    """Regions of magnitude 1e-30, 1e-36 (near fp32's normal floor), 1, 1e30: each is filtered to
    relative accuracy against its own neighbourhood, not the stream maximum."""
    p = nsh.FirCascadePlan(C5)
    n_out = 16 * 1024
    x = orc.synth(16 * n_out, 11)
    seg = x.size // 8
    for i, s in enumerate([1e-30, 1.0, 1e30, 1e-36, 1e20, 1e-20, 1.0, 1e-30]):
        x[i * seg:(i + 1) * seg] *= np.float32(s)
    y, _ = run_pfft(torch_cuda, p, x, n_out)
    ry = ref_chain(x, C5)
    ok, nbad = _local_ok(y, ry)
    assert ok, nbad


def test_c5_zero_and_empty(torch_cuda):
    p = nsh.FirCascadePlan(C5)
    y, _ = run_pfft(torch_cuda, p, np.zeros(16 * 5000, np.complex64), 5000)
    assert not np.any(y)
    y, _ = run_pfft(torch_cuda, p, np.zeros(0, np.complex64), 0)  # n_out = 0: no launch, no error
    assert y.size == 0


@pytest.mark.parametrize("log2n", [26, 28])
def test_c5_windowed_large(torch_cuda, log2n):
    """2^26 inputs (2^22 outputs, every workgroup busy with ~40 frames) and BASELINE C5's full
    2^28 (as bench.py's c5_fused leg): windows at the start, the middle (workgroup boundaries)
    and the tail against the oracle with their histories."""
    torch = torch_cuda
    p = nsh.FirCascadePlan(C5)
    n_out = 1 << (log2n - 4)
    dx = torch.empty(16 * n_out, dtype=torch.complex64, device="cuda")
    nsh.synth(dx, 16 * n_out, 0)
    dy = torch.empty(n_out, dtype=torch.complex64, device="cuda")
    dho = torch.empty(1890, dtype=torch.complex64, device="cuda")
    p(dx, None, dho, dy, n_out)
    torch.cuda.synchronize()
    y = dy.cpu().numpy()
    nf = (n_out + 392) // 393
    fpw = (nf + 255) // 256  # frames per workgroup (one workgroup per CU at D = 16)
    for start in (0, 393 * 164 - 7, 393 * fpw - 1500, 393 * fpw * 129 - 10, n_out // 2 + 12345, n_out - 3000):
        m = 3000 if start + 3000 <= n_out else n_out - start
        lo = max(0, start - 128)  # 128 outputs of lead-in cover the 1890-sample support
        xs = orc.synth(16 * (start + m - lo), 16 * lo)
        ry = ref_chain(xs, C5)[start - lo:]
        ok, err, scale = orc.tol_ok(y[start:start + m], ry)
        assert ok, (start, err, scale)


def test_c5_odd_sample_offsets(torch_cuda):
    """The fused chain on input, output and history pointers at odd sample offsets (8-B but not
    16-B aligned) into larger buffers, three calls with the history handed on, output guards
    untouched; against the oracle's staged chain."""
    torch = torch_cuda
    p = nsh.FirCascadePlan(C5)
    sizes = [3, 1000, 40_001]
    n_total = sum(sizes)
    x = orc.synth(16 * n_total, 91)
    dx = torch.zeros(16 * n_total + 3, dtype=torch.complex64, device="cuda")
    dx[1:1 + 16 * n_total] = torch.from_numpy(x).cuda()
    guard = complex(7.0, -7.0)
    dy = torch.full((n_total + 3,), guard, dtype=torch.complex64, device="cuda")
    hs = [torch.zeros(1891, dtype=torch.complex64, device="cuda") for _ in range(2)]
    pos, cur = 0, 0
    for i, m in enumerate(sizes):
        p(dx[1 + 16 * pos:], None if i == 0 else hs[cur][1:], hs[cur ^ 1][1:], dy[1 + pos:], m)
        cur ^= 1
        pos += m
    torch.cuda.synchronize()
    y = dy.cpu().numpy()
    assert y[0] == guard and np.all(y[1 + n_total:] == guard)
    ok, err, scale = orc.tol_ok(y[1:1 + n_total], ref_chain(x, C5))
    assert ok, (err, scale)


def test_c5_many_calls_ring_offsets(torch_cuda):
    """The flowgraph pattern: one device input buffer read at advancing offsets (multiples of 16
    samples), outputs written at arbitrary 8-B-aligned offsets of one buffer, ping-pong
    histories, a side stream; 300 calls of random sizes (1 .. 3000 outputs)."""
    torch = torch_cuda
    p = nsh.FirCascadePlan(C5)
    rng = np.random.default_rng(5)
    sizes = rng.integers(1, 3000, 300)
    n_total = int(sizes.sum())
    x = orc.synth(16 * n_total, 77)
    ry = ref_chain(x, C5)
    dx = torch.from_numpy(x).cuda()
    dy = torch.full((n_total + 1,), complex(5.0, 5.0), dtype=torch.complex64, device="cuda")
    hs = [torch.empty(1890, dtype=torch.complex64, device="cuda") for _ in range(2)]
    s = torch.cuda.Stream()
    pos, cur = 0, 0
    with torch.cuda.stream(s):
        for i, m in enumerate(sizes):
            m = int(m)
            p(dx[16 * pos:], None if i == 0 else hs[cur], hs[cur ^ 1], dy[1 + pos:], m, stream=s)
            cur ^= 1
            pos += m
    s.synchronize()
    y = dy.cpu().numpy()[1:]
    ok, err, scale = orc.tol_ok(y, ry)
    assert ok, (err, scale, int(np.argmax(np.abs(y - ry))))


@pytest.mark.parametrize("decim", [8, 16])
@pytest.mark.parametrize("ntaps", [1, 31, 127, 511, 2049])
def test_firplan_auto_pfft(torch_cuda, decim, ntaps, pfft_form):
    """nsh_fir_plan_create(AUTO) routes decim 8 and 16 to the polyphase-FFT kernel (one-stage
    cascade): same nsh_fir_ccf contract (ntaps-1 history, ping-pong), against the oracle over
    calls of several sizes."""
    torch = torch_cuda
    if (ntaps - 1 + decim - 1) // decim > 256:
        with pytest.raises(nsh.NshError):
            nsh.FirPlan(np.ones(ntaps, np.float32), decim)  # decim 16 has no other form
        return
    h = np.asarray(__import__("scipy.signal", fromlist=["firwin"]).firwin(ntaps, 0.8 / decim), np.float32) \
        if ntaps > 1 else np.array([0.75], np.float32)
    plan = nsh.FirPlan(h, decim)
    assert plan.algo == nsh.FIR_PFFT and plan.kernel == (KERNEL16[pfft_form] if decim == 16 else "k_fir_pfft<8,1>")
    cuts = [0, 3, 500, 501, 9000, 40000]
    x = orc.synth(decim * cuts[-1], ntaps)
    ref = orc.fir_ccf(x, h, decim)
    hist = torch.zeros(max(ntaps - 1, 1), dtype=torch.complex64, device="cuda")
    hout = torch.zeros_like(hist)
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        dx = torch.from_numpy(x[decim * a:decim * b]).cuda()
        dy = torch.empty(b - a, dtype=torch.complex64, device="cuda")
        plan(dx, hist if a else 0, hout, dy, b - a)
        torch.cuda.synchronize()
        hist, hout = hout, hist
        parts.append(dy.cpu().numpy())
    y = np.concatenate(parts)
    ok, err, scale = tol_pfft(y, ref, x, [(h, decim)])
    assert ok, (decim, ntaps, err, scale)
    ok, err, scale = orc.tol_ok(y[500:], ref[500:])  # past the zero-history transient: the plain rule
    assert ok, (decim, ntaps, err, scale)
