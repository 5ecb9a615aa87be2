"""Kernel-level timing of the plan-based FFT at every size, every comparison interleaved in one
process. Each time is the kernel's own: an event pair armed with nsh_time_next_launch, recorded by the
launch itself.

  nsh_fft_c2c       forward, N = 16 .. 8192, 2^26 samples per launch: plain and Hann window + shift
  nsh_fft1024_c2c   k_fft1024 over the same samples
  nsh_copy          over the same 16 B per sample (8 B read, 8 B written)
  --cap-sweep       also an all-ones-window plan (k_fft<N> at every size) under grid caps of 512 .. 16384
                    workgroups (nsh_fft_plan_grid_cap)
  --io-ab           for N <= 256 also both ways of moving the samples (NSH_FFT_IO=strided: pass 1's
                    register layout loaded directly; linear: coalesced accesses through the LDS image)

Per leg: a warm-up of at least 0.5 s of that leg, then the median over the rounds of the mean kernel
time of `reps` calls (us), the spread (min, max) of those rounds, GS/s, and the fraction of 8 TB/s on
16 B per sample. The legs alternate round by round.

Usage: python tools/fft_bench.py [--rounds R] [--reps K] [--log2n N] [--io-ab] [--cap-sweep] [--out profiles/fft_bench.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from newsched_amd import nsh
from tools.pfb_bench import WARMUP_S, KernelTimer, interleaved, summary

SIZES = [16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192]
IO_AB_MAX = 256
CAPS = [512, 1024, 2048, 4096, 8192, 16384]


def plan_with_io(io, *args, **kw):
    old = os.environ.get("NSH_FFT_IO")
    os.environ["NSH_FFT_IO"] = io
    try:
        return nsh.FftPlan(*args, **kw)
    finally:
        if old is None:
            del os.environ["NSH_FFT_IO"]
        else:
            os.environ["NSH_FFT_IO"] = old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=26, help="samples per launch")
    ap.add_argument("--io-ab", action="store_true")
    ap.add_argument("--cap-sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "fft_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fft_bench needs a GPU"
    s = torch.cuda.Stream()
    n = 1 << a.log2n
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    y = torch.empty_like(x)
    nsh.synth(x, n, 0, stream=s)
    s.synchronize()
    timer = KernelTimer()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "warmup_s": WARMUP_S,
           "n_samples": n, "timing": "kernel time from the launch's own event pair (nsh_time_next_launch)", "fft": {}}

    for N in SIZES:
        hann = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)).astype(np.float32)
        plans = {"plain": nsh.FftPlan(N), "hann_shift": nsh.FftPlan(N, False, hann, True)}
        if a.io_ab and N <= IO_AB_MAX:
            plans["plain_strided"] = plan_with_io("strided", N)
            plans["plain_linear"] = plan_with_io("linear", N)
        if a.cap_sweep:
            for cap in CAPS:
                plans["win_cap%d" % cap] = nsh.FftPlan(N, False, np.ones(N, np.float32))
                plans["win_cap%d" % cap].grid_cap(cap)
        legs = {k: [lambda p=p: p(x, y, n // N, stream=s)] for k, p in plans.items()}
        legs["fft1024"] = [lambda: nsh.fft1024(x, y, n // 1024, stream=s)]
        legs["copy"] = [lambda: nsh.copy(x, y, 8 * n, stream=s)]
        t = interleaved(legs, a.rounds, a.reps, timer)
        r = {k: summary(t[k], n, 16) for k in legs}
        r["kernel"] = {k: p.kernel for k, p in plans.items()}
        r["tile"] = plans["plain"].tile
        for k in plans:
            r[k + "_over_fft1024"] = round(r[k]["us"] / r["fft1024"]["us"], 4)
        r["plain_over_copy"] = round(r["plain"]["us"] / r["copy"]["us"], 4)
        for p in plans.values():
            p.close()
        res["fft"][f"N{N}"] = r
        print(f"fft N={N}:", json.dumps(r), flush=True)

    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
