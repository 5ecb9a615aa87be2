"""What tests/test_gpu_pfft.py and tests/test_gpu_pfft_taps.py share: the two forms of the 16-phase
kernel as a fixture, BASELINE config C5, the composite filter, the oracle's stage-by-stage chain and
the runner of one nsh_fir_cascade_ccf call."""
import numpy as np
import pytest

from oracle import oracle as orc

KERNEL16 = {"2": "k_fir_pfft2<16>", "1": "k_fir_pfft<16,1>"}


@pytest.fixture(autouse=True, params=["2", "1"], ids=["form2", "form1"])
def pfft_form(request, monkeypatch):
    monkeypatch.setenv("NSH_PFFT_FORM", request.param)
    return request.param


def _firwin(n, cutoff):
    return np.asarray(__import__("scipy.signal", fromlist=["firwin"]).firwin(n, cutoff), np.float32)


C5 = [(_firwin(127, 0.45), 2)] * 4


def heq_of(stages):
    """The composite filter in float64 from the fp32 stage taps."""
    h = np.ones(1)
    dacc = 1
    for t, d in stages:
        u = np.zeros((t.size - 1) * dacc + 1)
        u[::dacc] = np.asarray(t, np.float64)
        h = np.convolve(h, u)
        dacc *= d
    return h


def heq_l1(stages):
    """sum |heq| of the composite filter (double)."""
    return float(np.abs(heq_of(stages)).sum())


def ref_chain(x, stages):
    y = x
    for h, d in stages:
        y = orc.fir_ccf(y, h, d)
    return y


def run_pfft(torch, plan, x, n_out, hist=None, want_hist=True):
    assert x.size == plan.decim * n_out
    dx = torch.from_numpy(np.ascontiguousarray(x, np.complex64)).cuda() if x.size else \
        torch.zeros(1, dtype=torch.complex64, device="cuda")
    dh = torch.from_numpy(np.ascontiguousarray(hist, np.complex64)).cuda() if hist is not None else None
    dho = torch.full((plan.hist_len,), complex(9.0, 9.0), dtype=torch.complex64, device="cuda") if want_hist else None
    dy = torch.full((max(n_out, 1),), complex(7.0, 7.0), dtype=torch.complex64, device="cuda")
    plan(dx, dh, dho, dy, n_out)
    torch.cuda.synchronize()
    return dy.cpu().numpy()[:n_out], (dho.cpu().numpy() if want_hist else None)
