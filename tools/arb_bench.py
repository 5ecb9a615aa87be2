"""Kernel-level timing of the arbitrary-rate resampler, every comparison interleaved in one process. Each
time is the kernel's own: an event pair armed with nsh_time_next_launch, recorded by the launch itself.

  nsh_arb_resamp_ccf  at (rate, F, L) in LEGS, on about 2^log2n samples in and out together, phase 0
  nsh_copy            moving the same number of bytes, 8 (n_in + n_out): 4 (n_in + n_out) read and written
  nsh_resamp_ccf      for the two legs whose rate is 32 / D with F = 32: the same taps and data with
                      I = 32 (the step is D whole filter steps, mu = 0: the same outputs)

Per leg: a warm-up of at least 0.5 s of that leg, then the median over the rounds of the mean kernel
time of `reps` calls (us), the spread (min, max) of those rounds, input and output GS/s, the fraction
of 8 TB/s on 8 (n_in + n_out) bytes and the ratio to the copy. The legs alternate round by round.

Usage: python tools/arb_bench.py [--rounds R] [--reps K] [--log2n N] [--out profiles/arb_bench.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from newsched_amd import nsh
from tools.pfb_bench import WARMUP_S, KernelTimer, interleaved
from tools.resamp_bench import summary

# (name, rate, F, L, D of the rational resampler with I = F that computes the same, or None)
LEGS = [("160/147", 160 / 147, 32, 384, None), ("147/160", 147 / 160, 32, 384, None),
        ("32/21", 32 / 21, 32, 384, 21), ("32/63", 32 / 63, 32, 384, 63),
        ("4", 4.0, 32, 384, None), ("1/4", 0.25, 32, 384, None), ("64", 64.0, 32, 384, None),
        ("1/64", 1 / 64, 32, 2048, None)]


def lowpass(L, F, rate):
    k = np.arange(L) - (L - 1) / 2.0
    t = np.hamming(L) * np.sinc(0.8 * k / F * min(1.0, rate))
    return (F * t / t.sum()).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=27, help="input and output samples together")
    ap.add_argument("--out", default=os.path.join("profiles", "arb_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "arb_bench needs a GPU"
    s = torch.cuda.Stream()
    n = 1 << a.log2n
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    y = torch.empty_like(x)
    nsh.synth(x, n, 0, stream=s)
    s.synchronize()
    timer = KernelTimer()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "warmup_s": WARMUP_S,
           "samples_in_and_out": n, "timing": "kernel time from the launch's own event pair (nsh_time_next_launch)",
           "counters": "none taken", "arb": {}}

    for name, rate, F, L, D in LEGS:
        taps = lowpass(L, F, rate)
        plan = nsh.ArbPlan(taps, rate, F)
        n_in = int(n / (1 + plan.rate_effective))
        if D is not None:
            n_in -= n_in % D
        n_out, consumed, _ = plan.span(0, n_in, 2 ** 31 - 1)
        assert consumed == n_in and n_out <= n
        hin = torch.zeros(max(plan.history, 1), dtype=torch.complex64, device="cuda")
        hout = torch.zeros_like(hin)
        legs = {
            "arb": [lambda: plan(x, n_in, hin, hout, y, n_out, 0, stream=s)],
            "copy": [lambda: nsh.copy(x, y, 4 * (n_in + n_out), stream=s)],
        }
        rs = None
        if D is not None:
            assert plan.step == D << 32 and n_out == n_in // D * F
            rs = nsh.ResampPlan(taps, F, D)
            rhin = torch.zeros(max(rs.history, 1), dtype=torch.complex64, device="cuda")
            rhout = torch.zeros_like(rhin)
            legs["resamp"] = [lambda: rs(x, rhin, rhout, y, n_in // D, stream=s)]
        t = interleaved(legs, a.rounds, a.reps, timer)
        r = {k: summary(v, n_in, n_out) for k, v in t.items()}
        r["kernel"] = plan.kernel
        r["outputs_per_workgroup"] = plan.tile
        r["rate_effective"] = plan.rate_effective
        r["nfilt"], r["ntaps"], r["taps_per_output"] = F, L, -(-L // F)
        r["n_in"], r["n_out"] = n_in, n_out
        r["arb_over_copy"] = round(r["arb"]["us"] / r["copy"]["us"], 4)
        if rs is not None:
            r["resamp_kernel"] = rs.kernel
            r["arb_over_resamp"] = round(r["arb"]["us"] / r["resamp"]["us"], 4)
            rs.close()
        plan.close()
        res["arb"][f"r{name}_F{F}_L{L}"] = r
        print(f"arb r={name} F={F} L={L}:", json.dumps(r), flush=True)

    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
