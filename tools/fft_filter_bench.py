"""Kernel-level timing of fft_filter_ccc (k_fft_xlat<N, 1, false>) against its comparators, every comparison
interleaved in one process. Each time is the kernel's own: an event pair armed with
nsh_time_next_launch, recorded by the launch itself.

  nsh_fft_filter_ccc  L = 127, 161, 162, 512, 1024, 2048, 4096 taps on 2^26 samples, under both candidate size
                      rules: rule2, the smallest N >= 2 pow2ceil(L), and rule4, N >= 4 pow2ceil(L), both
                      at least 1024 and at most 8192 (where rule4 would need more it is the same plan as
                      rule2 and is not run again)
  nsh_fft_c2c         forward, at the same N over the same samples
  nsh_copy            over the same 16 B per sample (8 B read, 8 B written)
  nsh_fir_ccf(AUTO)   the real parts of the same taps, those L up to 1024 and 257 on the same samples
                      (161 is the last tap count AUTO gives to k_fir_mfma12, 162 the first it does not); at
                      L = 2048 and 4096 on 2^-4 of the stream, the time scaled by 16 ("scaled": true)
  --cap-sweep         also every N at L = 127 under grid caps of 256 .. 16384 workgroups
                      (nsh_fft_filter_grid_cap)

Per leg: a warm-up of at least 0.5 s of that leg, then the median over the rounds of the mean kernel
time of `reps` calls (us), the spread (min, max) of those rounds, GS/s, and the fraction of 8 TB/s on
16 B per output. The legs alternate round by round.

Usage: python tools/fft_filter_bench.py [--rounds R] [--reps K] [--log2n N] [--cap-sweep] [--out profiles/fft_filter_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from newsched_amd import nsh
from tools.pfb_bench import WARMUP_S, KernelTimer, interleaved, summary

TAPS = [127, 161, 162, 512, 1024, 2048, 4096]
FIR_TAPS = [127, 161, 162, 257, 512, 1024, 2048, 4096]
FIR_FULL_MAX = 1024  # nsh_fir_ccf above this: a 16th of the stream, scaled
SIZES = [1024, 2048, 4096, 8192]
CAPS = [256, 512, 1024, 2048, 4096, 8192, 16384]


class CallTimer(KernelTimer):
    """KernelTimer for calls of one entry point each, whatever the launches inside: nsh_fir_ccf's MFMA
    forms launch twice, the pair's start recorded by the first launch and its stop by the last."""

    def __call__(self, calls):
        before, after = C.c_uint64(0), C.c_uint64(0)
        nsh.check(self.lib.nsh_timed_launches(C.byref(before)))
        for i, fn in enumerate(calls):
            a, b = self._pair(i)
            nsh.check(self.lib.nsh_time_next_launch(a, b))
            fn()
        nsh.check(self.lib.nsh_timed_launches(C.byref(after)))
        assert after.value - before.value >= len(calls), "a call launched nothing"
        torch.cuda.synchronize()
        tot = 0.0
        for i in range(len(calls)):
            ms = C.c_float(0)
            nsh.check(self.lib.nsh_event_elapsed_ms(self.pairs[i][0], self.pairs[i][1], C.byref(ms)))
            tot += ms.value
        return 1e3 * tot


def size_rule(L, k):
    """The smallest N >= k pow2ceil(L) among the kernel's sizes (the largest where none is)."""
    p = 1
    while p < L:
        p *= 2
    return min(max(k * p, 1024), 8192)


def lowpass(L):
    k = np.arange(L) - (L - 1) / 2.0
    t = np.hamming(L) * np.sinc(0.2 * k) if L > 1 else np.ones(1)
    return (t / t.sum()).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=26, help="samples per launch")
    ap.add_argument("--cap-sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "fft_filter_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fft_filter_bench needs a GPU"
    s = torch.cuda.Stream()
    n = 1 << a.log2n
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    y = torch.empty_like(x)
    hin = torch.zeros(4096, dtype=torch.complex64, device="cuda")
    hout = torch.zeros(4096, dtype=torch.complex64, device="cuda")
    nsh.synth(x, n, 0, stream=s)
    s.synchronize()
    timer = CallTimer()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "warmup_s": WARMUP_S,
           "n_samples": n, "timing": "kernel time from the call's own event pair (nsh_time_next_launch); nsh_fir_ccf's MFMA forms "
                     "are two launches under one pair",
           "fft_filter": {}, "fir_ccf_auto": {}}

    for L in FIR_TAPS:
        h = lowpass(L)
        legs, plans = {}, {}
        scale = 1 if L <= FIR_FULL_MAX else 16
        fir = nsh.FirPlan(h, 1, nsh.FIR_AUTO)
        legs["fir_ccf_auto"] = [lambda: fir(x, hin, hout, y, n // scale, stream=s)]
        if L in TAPS:
            for name, k in (("rule2", 2), ("rule4", 4)):
                N = size_rule(L, k)
                if name == "rule4" and N == size_rule(L, 2):
                    continue
                plans[name] = nsh.FftFilterPlan(h.astype(np.complex64), N)
                legs[name] = [lambda p=plans[name]: p(x, hin, hout, y, n, stream=s)]
                fp = plans["fft_" + name] = nsh.FftPlan(N, False, np.ones(N, np.float32))  # k_fft<N> at every size
                legs["fft_" + name] = [lambda p=fp, N=N: p(x, y, n // N, stream=s)]
            legs["copy"] = [lambda: nsh.copy(x, y, 8 * n, stream=s)]
        t = interleaved(legs, a.rounds, a.reps, timer)
        f = summary([u * scale for u in t["fir_ccf_auto"]], n)
        f.update(kernel=fir.kernel, scaled=scale != 1, stream_fraction=1.0 / scale)
        res["fir_ccf_auto"][f"L{L}"] = f
        print(f"fir_ccf(AUTO) L={L}:", json.dumps(f), flush=True)
        if L in TAPS:
            r = {"copy": summary(t["copy"], n, 16)}
            for name in ("rule2", "rule4"):
                if name not in plans:
                    continue
                p = plans[name]
                e = summary(t[name], n, 16)
                e.update(fft_size=p.fft_size, valid=p.valid, tile=p.tile, kernel=p.kernel,
                         fft_c2c=summary(t["fft_" + name], n, 16))
                e["over_copy"] = round(e["us"] / r["copy"]["us"], 4)
                e["over_fft_c2c"] = round(e["us"] / e["fft_c2c"]["us"], 4)
                e["over_fir_ccf_auto"] = round(e["us"] / f["us"], 5)
                r[name] = e
            d = nsh.FftFilterPlan(h.astype(np.complex64))
            r["default_fft_size"] = d.fft_size  # what fft_size = 0 gives
            d.close()
            res["fft_filter"][f"L{L}"] = r
            print(f"fft_filter L={L}:", json.dumps(r), flush=True)
        fir.close()
        for p in plans.values():
            p.close()

    if a.cap_sweep:
        res["cap_sweep"] = {}
        h = lowpass(127).astype(np.complex64)
        for N in SIZES:
            plans = {}
            for cap in CAPS:
                plans["cap%d" % cap] = nsh.FftFilterPlan(h, N)
                plans["cap%d" % cap].grid_cap(cap)
            legs = {k: [lambda p=p: p(x, hin, hout, y, n, stream=s)] for k, p in plans.items()}
            t = interleaved(legs, a.rounds, a.reps, timer)
            r = {k: summary(t[k], n, 16) for k in legs}
            res["cap_sweep"][f"N{N}"] = r
            print(f"cap sweep N={N}:", json.dumps({k: v["us"] for k, v in r.items()}), flush=True)
            for p in plans.values():
                p.close()

    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
