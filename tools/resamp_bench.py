"""Kernel-level timing of the rational resampler, every comparison interleaved in one process. Each
time is the kernel's own: an event pair armed with nsh_time_next_launch, recorded by the launch itself.

  nsh_resamp_ccf      at (I, D, L) in LEGS, on about 2^log2n samples in and out together
  nsh_copy            moving the same number of bytes, 8 (n_in + n_out): 4 (n_in + n_out) read and written
  nsh_fir_xlat_ccf    for the two I = 1 legs: the same taps and data at freq_norm = 0 (the same outputs)

Per leg: a warm-up of at least 0.5 s of that leg, then the median over the rounds of the mean kernel
time of `reps` calls (us), the spread (min, max) of those rounds, input and output GS/s, the fraction
of 8 TB/s on 8 (n_in + n_out) bytes and the ratio to the copy. The legs alternate round by round.

Usage: python tools/resamp_bench.py [--rounds R] [--reps K] [--log2n N] [--out profiles/resamp_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from newsched_amd import nsh
from tools.pfb_bench import HBM_BPS, WARMUP_S, KernelTimer, interleaved

LEGS = [(2, 1, 63), (4, 1, 127), (3, 2, 95), (2, 3, 95), (4, 5, 159), (1, 4, 127), (64, 1, 1024), (1, 64, 1024)]


def summary(us, n_in, n_out):
    med = statistics.median(us)
    return {"us": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
            "spread": round((max(us) - min(us)) / med, 4), "GS/s_in": round(n_in / med / 1e3, 2),
            "GS/s_out": round(n_out / med / 1e3, 2),
            "hbm_frac": round(8 * (n_in + n_out) / (med * 1e-6) / HBM_BPS, 4)}


def lowpass(L, I, D):
    k = np.arange(L) - (L - 1) / 2.0
    t = np.hamming(L) * np.sinc(0.8 * k / max(I, D))
    return (I * t / t.sum()).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=27, help="input and output samples together")
    ap.add_argument("--out", default=os.path.join("profiles", "resamp_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "resamp_bench needs a GPU"
    s = torch.cuda.Stream()
    n = 1 << a.log2n
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    y = torch.empty_like(x)
    nsh.synth(x, n, 0, stream=s)
    s.synchronize()
    timer = KernelTimer()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "warmup_s": WARMUP_S,
           "samples_in_and_out": n, "timing": "kernel time from the launch's own event pair (nsh_time_next_launch)",
           "resamp": {}}

    for I, D, L in LEGS:
        taps = lowpass(L, I, D)
        units = n // (I + D)
        n_in, n_out = units * D, units * I
        plan = nsh.ResampPlan(taps, I, D)
        hin = torch.zeros(max(plan.history, 1), dtype=torch.complex64, device="cuda")
        hout = torch.zeros_like(hin)
        legs = {
            "resamp": [lambda: plan(x, hin, hout, y, units, stream=s)],
            "copy": [lambda: nsh.copy(x, y, 4 * (n_in + n_out), stream=s)],
        }
        xl = None
        if I == 1:
            xl = nsh.FirXlatPlan(taps, D, 0.0)
            legs["xlat"] = [lambda: xl(x, hin, hout, y, units, 0, stream=s)]
        t = interleaved(legs, a.rounds, a.reps, timer)
        r = {k: summary(v, n_in, n_out) for k, v in t.items()}
        r["kernel"] = plan.kernel
        r["units_per_workgroup"] = plan.tile
        r["taps_per_output"] = -(-L // I)
        r["n_in"], r["n_out"] = n_in, n_out
        r["resamp_over_copy"] = round(r["resamp"]["us"] / r["copy"]["us"], 4)
        if xl is not None:
            r["xlat_kernel"] = xl.kernel
            r["resamp_over_xlat"] = round(r["resamp"]["us"] / r["xlat"]["us"], 4)
            xl.close()
        plan.close()
        res["resamp"][f"I{I}_D{D}_L{L}"] = r
        print(f"resamp I={I} D={D} L={L}:", json.dumps(r), flush=True)

    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
