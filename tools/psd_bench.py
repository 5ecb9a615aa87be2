"""Kernel-level timing of psd_vcf (k_psd<N, LIN>, and k_psd_sum past one segment) against its
comparators, every comparison interleaved in one process on the same 2^26 input samples. Each time is
the call's own: an event pair armed with nsh_time_next_launch, its start recorded by the call's first
launch and its stop by the last.

  nsh_psd_cf     N in {64, 1024, 4096, 8192} x K in {1, 16, 1024} and the single-spectrum case
                 K = min(2^26 / N, 65536), Hann window, scale 1 / K, linear; where K exceeds the plan's
                 segment P also with P = K (no segmentation, NSH_PSD_SEGMENT=0 at plan creation)
  nsh_fft_c2c    forward, Hann window, the same frames (16 B per sample)
  nsh_copy       the same input bytes (8 B read, 8 B written per sample)
  --sweep        K = 1024 and the single-spectrum K under P in {4 .. 256} (NSH_PSD_SEGMENT), and
                 K in {1, 16, single} under grid caps of 256 .. 16384 workgroups (nsh_psd_grid_cap),
                 and K = 32, 33, 48, 64 at N = 1024: both sides of the step from one segment to two

Per leg: a warm-up of at least 0.5 s of that leg, then the median over the rounds of the mean kernel
time of `reps` calls (us), the spread (min, max) of those rounds, GS/s, and the fraction of 8 TB/s on
8 + 4 / K bytes per sample (16 for the FFT and the copy). The legs alternate round by round, except
the P = K legs: they take 2 to 107 ms a call, and a 0.1 ms call timed in rotation with one read
12 to 15 % slower than among its like, so they are timed on their own after the others (3 rounds of
1 call).

Usage: python tools/psd_bench.py [--rounds R] [--reps K] [--log2n N] [--sweep] [--out profiles/psd_bench.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from newsched_amd import nsh
from tools.fft_filter_bench import CallTimer
from tools.pfb_bench import WARMUP_S, interleaved, summary

SIZES = [64, 1024, 4096, 8192]
NAVG = [1, 16, 1024]
SEGMENTS = [4, 8, 16, 32, 64, 256]
CAPS = [256, 512, 1024, 2048, 4096, 8192, 16384]


def hann(N):
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)).astype(np.float32)


def psd_plan(N, K, segment=None):
    """A plan with the default segment, or with P = segment (0: P = K)."""
    if segment is not None:
        os.environ["NSH_PSD_SEGMENT"] = str(segment)
    try:
        return nsh.PsdPlan(N, K, hann(N))
    finally:
        os.environ.pop("NSH_PSD_SEGMENT", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=26, help="input samples per call")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "psd_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "psd_bench needs a GPU"
    s = torch.cuda.Stream()
    n = 1 << a.log2n
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    y = torch.empty_like(x)
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    nsh.synth(x, n, 0, stream=s)
    s.synchronize()
    timer = CallTimer()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "warmup_s": WARMUP_S,
           "n_samples": n, "timing": "kernel time from the call's own event pair (nsh_time_next_launch); past one segment "
                     "nsh_psd_cf is two launches under one pair",
           "psd": {}}

    def shapes(N):
        return NAVG + [min(n // N, 65536)]

    for N in SIZES:
        fft = nsh.FftPlan(N, False, hann(N))
        for K in shapes(N):
            nvec = n // (N * K)
            used = nvec * N * K  # samples the call reads
            plans = {"psd": psd_plan(N, K)}
            legs = {"psd": [lambda p=plans["psd"]: p(x, out, nvec, stream=s)]}
            legs["fft_c2c"] = [lambda: fft(x, y, used // N, stream=s)]
            legs["copy"] = [lambda: nsh.copy(x, y, 8 * used, stream=s)]
            t = interleaved(legs, a.rounds, a.reps, timer)
            if K > plans["psd"].segment:
                plans["psd_noseg"] = psd_plan(N, K, 0)
                t.update(interleaved({"psd_noseg": [lambda p=plans["psd_noseg"]: p(x, out, nvec, stream=s)]}, 3, 1, timer))
            r = {"nvec": nvec, "samples": used, "fft_c2c": summary(t["fft_c2c"], used, 16), "copy": summary(t["copy"], used, 16)}
            for k, p in plans.items():
                e = summary(t[k], used, 8 + 4.0 / K)
                e.update(segment=p.segment, tile=p.tile, kernel=p.kernel)
                e["over_copy"] = round(e["us"] / r["copy"]["us"], 4)
                e["over_fft_c2c"] = round(e["us"] / r["fft_c2c"]["us"], 4)
                r[k] = e
                p.close()
            res["psd"][f"N{N}_K{K}"] = r
            print(f"psd N={N} K={K}:", json.dumps(r), flush=True)
        fft.close()

    if a.sweep:
        res["segment_sweep"], res["cap_sweep"] = {}, {}
        for N in SIZES:
            for K in shapes(N)[2:]:
                nvec = n // (N * K)
                plans = {"P%d" % P: psd_plan(N, K, P) for P in SEGMENTS if P < K}
                legs = {k: [lambda p=p: p(x, out, nvec, stream=s)] for k, p in plans.items()}
                t = interleaved(legs, a.rounds, a.reps, timer)
                r = {k: summary(t[k], nvec * N * K, 8 + 4.0 / K) for k in legs}
                res["segment_sweep"][f"N{N}_K{K}"] = r
                print(f"segment sweep N={N} K={K}:", json.dumps({k: v["us"] for k, v in r.items()}), flush=True)
                for p in plans.values():
                    p.close()
            for K in (1, 16, shapes(N)[3]):
                nvec = n // (N * K)
                plans = {}
                for cap in CAPS:
                    plans["cap%d" % cap] = psd_plan(N, K)
                    plans["cap%d" % cap].grid_cap(cap)
                legs = {k: [lambda p=p: p(x, out, nvec, stream=s)] for k, p in plans.items()}
                t = interleaved(legs, a.rounds, a.reps, timer)
                r = {k: summary(t[k], nvec * N * K, 8 + 4.0 / K) for k in legs}
                res["cap_sweep"][f"N{N}_K{K}"] = r
                print(f"cap sweep N={N} K={K}:", json.dumps({k: v["us"] for k, v in r.items()}), flush=True)
                for p in plans.values():
                    p.close()

        plans = {"K%d" % K: psd_plan(1024, K) for K in (32, 33, 48, 64)}
        legs = {k: [lambda p=p: p(x, out, n // (1024 * p.navg), stream=s)] for k, p in plans.items()}
        t = interleaved(legs, a.rounds, a.reps, timer)
        r = {k: dict(summary(t[k], n // (1024 * p.navg) * 1024 * p.navg, 8 + 4.0 / p.navg), segment=p.segment)
             for k, p in plans.items()}
        res["segment_step"] = {"N1024": r}
        print("segment step N=1024:", json.dumps({k: (v["us"], v["segment"]) for k, v in r.items()}), flush=True)
        for p in plans.values():
            p.close()

    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
