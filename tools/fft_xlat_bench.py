"""Kernel-level timing of freq_xlating_fft_filter_ccc (k_fft_xlat<N, D>) against its comparators, every
comparison interleaved in one process. Each time is the call's own: an event pair armed with
nsh_time_next_launch, recorded by the launch itself.

Cases (D, L) on 2^26 inputs: D = 1, 2, 4, 8, 16, 64 at 127 taps, (16, 255), (64, 1024), (8, 2048),
(16, 4096); real low-pass taps of cutoff 0.8 / D, tuned by 0.1137 cycles per sample.

  fft_xlat       nsh_fft_xlat_ccc, the default frame size
  copy           nsh_copy of the same bytes: the kernel reads 8 B per input and writes 8 / D, the
                 copy reads 4 + 4 / D and writes as many
  fft_filter     nsh_fft_filter_ccc on the same taps (decimation 1, untuned: 16 B per input)
  fir_xlat       nsh_fir_xlat_ccf, where L <= 1024
  staged         nsh_rotate_cc -> nsh_fir_ccf(AUTO, D), where D is 1, 2, 4, 8 or 16: two calls, their
                 kernel times added (the rotated stream makes a round trip through HBM)
  --rules        also D = 8 and 16 at 512, 1024 and 2048 taps under both size rules (rule2: the smallest
                 N >= 2 pow2ceil(L), rule4: N >= 4 pow2ceil(L), within 1024 .. 8192)
  --cap-sweep    also every N at L = 127, D = 8 under grid caps of 256 .. 16384 workgroups

Per leg: a warm-up of at least 0.5 s of that leg, then the median over the rounds of the mean kernel
time of `reps` calls (us), the spread (min, max) of those rounds, GS/s of input, and the fraction of
8 TB/s on the leg's bytes. The legs alternate round by round.

Usage: python tools/fft_xlat_bench.py [--rounds R] [--reps K] [--log2n N] [--rules] [--cap-sweep]
                                      [--out profiles/fft_xlat_bench.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from newsched_amd import nsh
from tools.fft_filter_bench import CallTimer, size_rule
from tools.pfb_bench import WARMUP_S, interleaved, lowpass, summary

CASES = [(1, 127), (2, 127), (4, 127), (8, 127), (16, 127), (64, 127), (16, 255), (64, 1024), (8, 2048), (16, 4096)]
FREQ = 0.1137
RULE_TAPS = [512, 1024, 2048]
SIZES = [1024, 2048, 4096, 8192]
CAPS = [256, 512, 1024, 2048, 4096, 8192, 16384]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=26, help="input samples per launch")
    ap.add_argument("--rules", action="store_true")
    ap.add_argument("--cap-sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "fft_xlat_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fft_xlat_bench needs a GPU"
    s = torch.cuda.Stream()
    n = 1 << a.log2n
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    y = torch.empty_like(x)
    tmp = torch.empty_like(x)
    hin = torch.zeros(4096, dtype=torch.complex64, device="cuda")
    hout = torch.zeros(4096, dtype=torch.complex64, device="cuda")
    nsh.synth(x, n, 0, stream=s)
    s.synchronize()
    timer = CallTimer()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "warmup_s": WARMUP_S,
           "n_inputs": n, "freq_norm": FREQ,
           "timing": "kernel time from the call's own event pair (nsh_time_next_launch); staged is two calls, added",
           "cases": {}}

    for D, L in CASES:
        h = lowpass(L, max(D, 2))
        hc = h.astype(np.complex64)
        n_out = n // D
        # nsh_copy writes what it reads: the kernel's 8 + 8 / D bytes per input are (4 + 4 / D) n read
        # and as many written
        copy_bytes = 4 * n + 4 * n // D
        plans = {"fft_xlat": nsh.FftXlatPlan(hc, D, FREQ), "fft_filter": nsh.FftFilterPlan(hc)}
        legs = {"fft_xlat": [lambda p=plans["fft_xlat"]: p(x, hin, hout, y, n_out, 0, stream=s)],
                "copy": [lambda b=copy_bytes: nsh.copy(x, y, b, stream=s)],
                "fft_filter": [lambda p=plans["fft_filter"]: p(x, hin, hout, y, n, stream=s)]}
        if L <= 1024:
            plans["fir_xlat"] = nsh.FirXlatPlan(h, D, FREQ)
            legs["fir_xlat"] = [lambda p=plans["fir_xlat"]: p(x, hin, hout, y, n_out, 0, stream=s)]
        if D <= 16:
            plans["staged"] = nsh.FirPlan(h, D, nsh.FIR_AUTO)
            inc = plans["fft_xlat"].phase_inc
            legs["staged"] = [lambda: nsh.rotate_cc(x, tmp, n, inc, 0, stream=s),
                              lambda p=plans["staged"]: p(tmp, hin, hout, y, n_out, stream=s)]
        t = interleaved(legs, a.rounds, a.reps, timer)
        p = plans["fft_xlat"]
        r = {"fft_xlat": summary(t["fft_xlat"], n, 8 + 8 / D), "copy": summary(t["copy"], n, 8 + 8 / D),
             "fft_filter": summary(t["fft_filter"], n, 16)}
        r["copy"]["bytes_read_and_written"] = 2 * copy_bytes
        r["fft_xlat"].update(fft_size=p.fft_size, overlap=p.overlap, valid=p.valid, tile=p.tile, kernel=p.kernel)
        r["fft_filter"].update(kernel=plans["fft_filter"].kernel)
        for k in ("fir_xlat", "staged"):
            if k in legs:
                r[k] = summary(t[k], n)
                r[k]["kernel"] = plans[k].kernel
        for k in ("copy", "fft_filter", "fir_xlat", "staged"):
            if k in r:
                r["fft_xlat"]["over_" + k] = round(r["fft_xlat"]["us"] / r[k]["us"], 4)
        res["cases"][f"D{D}_L{L}"] = r
        print(f"D={D} L={L}:", json.dumps(r), flush=True)
        for q in plans.values():
            q.close()

    if a.rules:
        res["rules"] = {}
        for D in (8, 16):
            for L in RULE_TAPS:
                hc = lowpass(L, D).astype(np.complex64)
                plans = {name: nsh.FftXlatPlan(hc, D, FREQ, fft_size=size_rule(L, k)) for name, k in (("rule2", 2), ("rule4", 4))}
                legs = {k: [lambda p=p: p(x, hin, hout, y, n // D, 0, stream=s)] for k, p in plans.items()}
                t = interleaved(legs, a.rounds, a.reps, timer)
                r = {k: dict(summary(t[k], n, 8 + 8 / D), fft_size=plans[k].fft_size) for k in legs}
                res["rules"][f"D{D}_L{L}"] = r
                print(f"rules D={D} L={L}:", json.dumps(r), flush=True)
                for p in plans.values():
                    p.close()

    if a.cap_sweep:
        res["cap_sweep"] = {}
        hc = lowpass(127, 8).astype(np.complex64)
        for N in SIZES:
            plans = {}
            for cap in CAPS:
                plans["cap%d" % cap] = nsh.FftXlatPlan(hc, 8, FREQ, fft_size=N)
                plans["cap%d" % cap].grid_cap(cap)
            legs = {k: [lambda p=p: p(x, hin, hout, y, n // 8, 0, stream=s)] for k, p in plans.items()}
            t = interleaved(legs, a.rounds, a.reps, timer)
            r = {k: summary(t[k], n, 9) for k in legs}
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
