"""GPU parity for the paths of the fp16x2 split in the FIR matrix-core kernels: both forms of the
per-chunk scale (packed multiply, ldexp for scale exponents above 127), the compile-time LDS
offsets of k_fir_mfma12's k-loop at every dispatched Q, and the same split in the decimators
(k_fir_mfma13). Each case against the CPU oracle on the same inputs, oracle.tol_ok."""
import numpy as np
import pytest
import scipy.signal as ss

from oracle import oracle as orc
from newsched_amd import nsh

pytestmark = pytest.mark.gpu


def _run(torch, plan, x, n_out, hist):
    dx = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    hin = torch.from_numpy(np.ascontiguousarray(hist)).cuda()
    hout = torch.zeros_like(hin)
    dy = torch.empty(n_out, dtype=torch.complex64, device="cuda")
    plan(dx, hin, hout, dy, n_out)
    torch.cuda.synchronize()
    return dy.cpu().numpy()


def test_fir_mfma_scale_multiply_and_ldexp(torch_cuda):
    """3-chunk segments at amplitudes 2^-120 (scale exponent 134 or 135: above 127, the ldexp
    form), 2^-100, 1 and 2^120 (the packed multiply), after a history at the first segment's
    amplitude: every segment meets the tolerance on its own scale, from 127 samples after its
    start (the first from its first sample)."""
    torch = torch_cuda
    h = ss.firwin(127, 0.2).astype(np.float32)
    seg = 3 * 2048
    amps = [np.float32(2.0 ** -120), np.float32(2.0 ** -100), np.float32(1.0), np.float32(2.0 ** 120)]
    x = orc.synth(len(amps) * seg, 33)
    for i, a in enumerate(amps):
        x[i * seg:(i + 1) * seg] *= a
    # 141 - (biased exponent of the largest magnitude) is the chunk's scale exponent
    top = float(max(np.abs(x[:seg].real).max(), np.abs(x[:seg].imag).max()))
    assert 141 - (int(np.floor(np.log2(top))) + 127) > 127, top
    hist = orc.synth(126, 4000) * amps[0]
    plan = nsh.FirPlan(h, 1, nsh.FIR_MFMA)
    assert plan.kernel == "k_fir_mfma12<5>", plan.kernel
    y = _run(torch, plan, x, x.size, hist)
    ref = orc.fir_ccf(x, h, hist=hist)
    for i in range(len(amps)):
        a, b = (i * seg + 127 if i else 0), (i + 1) * seg
        ok, err, scale = orc.tol_ok(y[a:b], ref[a:b])
        print("segment", i, "amplitude", float(amps[i]), "err", err, "scale", scale)
        assert ok, (i, err, scale)
    plan.close()


@pytest.mark.parametrize("ntaps,Q", [(33, 2), (65, 3), (97, 4), (127, 5), (161, 6)])
def test_fir_mfma12_every_q(torch_cuda, ntaps, Q):
    """k_fir_mfma12<Q> reads its A and B fragments at compile-time offsets from one base each:
    random taps (no near-zero tap hides a wrong offset), nonzero history, two full chunks and a
    ragged tail, the full output against the oracle."""
    torch = torch_cuda
    rng = np.random.default_rng(1000 + ntaps)
    h = rng.standard_normal(ntaps).astype(np.float32)
    n = 2 * 2048 + 300
    x = orc.synth(n, 17 * ntaps)
    hist = orc.synth(ntaps - 1, 5 * ntaps + 1)
    plan = nsh.FirPlan(h, 1, nsh.FIR_MFMA)
    assert plan.kernel == "k_fir_mfma12<%d>" % Q, plan.kernel
    y = _run(torch, plan, x, n, hist)
    ok, err, scale = orc.tol_ok(y, orc.fir_ccf(x, h, hist=hist))
    print("Q", Q, "err", err, "scale", scale)
    assert ok, (Q, err, scale)
    plan.close()


@pytest.mark.parametrize("decim,kernel", [(2, "k_fir_mfma13<2,5>"), (4, "k_fir_mfma13<4,3>")])
def test_fir_decim_shared_split(torch_cuda, decim, kernel):
    """The decimators split their samples with the same helpers: 127 taps at decim 2 and 4, three
    input chunks and 64 samples, nonzero history, against the oracle."""
    torch = torch_cuda
    h = ss.firwin(127, 0.2).astype(np.float32)
    n_in = 3 * 2048 + 64
    x = orc.synth(n_in, 29 + decim)
    hist = orc.synth(126, 900 + decim)
    plan = nsh.FirPlan(h, decim, nsh.FIR_MFMA)
    assert plan.kernel == kernel, plan.kernel
    y = _run(torch, plan, x, n_in // decim, hist)
    ok, err, scale = orc.tol_ok(y, orc.fir_ccf(x, h, decim, hist=hist))
    print("decim", decim, "err", err, "scale", scale)
    assert ok, (decim, err, scale)
    plan.close()
