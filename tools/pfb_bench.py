"""Kernel-level timing of the polyphase filterbank channelizer, every comparison interleaved in one
process. Each time is the kernel's own: an event pair armed with nsh_time_next_launch, recorded by the
launch itself.

  nsh_pfb_channelizer_ccf   at M in {4, 16, 64} with L = 8 M - 1 and with L = 127, on 2^26 inputs
  M x nsh_fir_xlat_ccf      the M FirXlatPlan(taps, M, c / M) launches that produce the same channels
                            (the sum of their M kernel times)
  nsh_copy                  over the same 16 B per input sample (8 B read, 8 B written)

Per leg: a warm-up of at least 0.5 s of that leg, then the median over the rounds of the mean kernel
time of `reps` calls (us), the spread (min, max) of those rounds, input GS/s, and for the channelizer
and the copy the fraction of 8 TB/s on 16 B per input sample. The legs alternate round by round.

Usage: python tools/pfb_bench.py [--rounds R] [--reps K] [--log2n N] [--out profiles/pfb_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from newsched_amd import nsh

HBM_BPS = 8e12
CASES = [(4, 31), (4, 127), (16, 127), (64, 511), (64, 127)]  # L = 8 M - 1 and L = 127 (the same case at M = 16)
WARMUP_S = 0.5


class KernelTimer:
    """Sum of the kernel times of the launches made by the calls passed to __call__ (one armed pair each)."""

    def __init__(self):
        self.lib = nsh.lib()
        self.pairs = []

    def _pair(self, i):
        while len(self.pairs) <= i:
            a, b = C.c_void_p(), C.c_void_p()
            nsh.check(self.lib.nsh_event_create(C.byref(a)))
            nsh.check(self.lib.nsh_event_create(C.byref(b)))
            self.pairs.append((a, b))
        return self.pairs[i]

    def __call__(self, calls):
        """calls: a list of functions of one launch each. Returns the summed kernel time in us."""
        before, after = C.c_uint64(0), C.c_uint64(0)
        nsh.check(self.lib.nsh_timed_launches(C.byref(before)))
        for i, fn in enumerate(calls):
            a, b = self._pair(i)
            nsh.check(self.lib.nsh_time_next_launch(a, b))
            fn()
        nsh.check(self.lib.nsh_timed_launches(C.byref(after)))
        assert after.value - before.value == len(calls), "a call was not exactly one launch"
        torch.cuda.synchronize()
        tot = 0.0
        for i in range(len(calls)):
            ms = C.c_float(0)
            nsh.check(self.lib.nsh_event_elapsed_ms(self.pairs[i][0], self.pairs[i][1], C.byref(ms)))
            tot += ms.value
        return 1e3 * tot


def interleaved(legs, rounds, reps, timer):
    """legs: {name: [one-launch functions]}. Returns {name: [us per round]}."""
    for calls in legs.values():  # warm-up: code objects, clocks
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < WARMUP_S:
            for fn in calls:
                fn()
            torch.cuda.synchronize()
    out = {k: [] for k in legs}
    for _ in range(rounds):
        for k, calls in legs.items():
            out[k].append(sum(timer(calls) for _ in range(reps)) / reps)
    return out


def summary(us, n_in, bytes_per_in=None):
    med = statistics.median(us)
    r = {"us": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
         "spread": round((max(us) - min(us)) / med, 4), "GS/s_in": round(n_in / med / 1e3, 2)}
    if bytes_per_in is not None:
        r["hbm_frac"] = round(bytes_per_in * n_in / (med * 1e-6) / HBM_BPS, 4)
    return r


def lowpass(L, M):
    k = np.arange(L) - (L - 1) / 2.0
    t = np.hamming(L) * np.sinc(0.8 * k / M)
    return (t / t.sum()).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=26, help="input samples")
    ap.add_argument("--out", default=os.path.join("profiles", "pfb_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pfb_bench needs a GPU"
    s = torch.cuda.Stream()
    n_in = 1 << a.log2n
    x = torch.empty(n_in, dtype=torch.complex64, device="cuda")
    y = torch.empty_like(x)
    yx = torch.empty(n_in // 4, dtype=torch.complex64, device="cuda")
    nsh.synth(x, n_in, 0, stream=s)
    s.synchronize()
    timer = KernelTimer()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "warmup_s": WARMUP_S,
           "n_in": n_in, "timing": "kernel time from the launch's own event pair (nsh_time_next_launch)", "pfb": {}}

    for M, L in CASES:
        taps = lowpass(L, M)
        n_out = n_in // M
        pfb = nsh.PfbPlan(taps, M)
        hin = torch.zeros(max(L - 1, 1), dtype=torch.complex64, device="cuda")
        hout = torch.zeros_like(hin)
        xl = [nsh.FirXlatPlan(taps, M, c / M) for c in range(M)]
        legs = {
            "pfb": [lambda: pfb(x, hin, hout, y, n_out, stream=s)],
            "xlat_x_M": [(lambda p=p: p(x, hin, hout, yx, n_out, 0, stream=s)) for p in xl],
            "copy": [lambda: nsh.copy(x, y, 8 * n_in, stream=s)],
        }
        t = interleaved(legs, a.rounds, a.reps, timer)
        r = {"pfb": summary(t["pfb"], n_in, 16), "xlat_x_M": summary(t["xlat_x_M"], n_in),
             "copy": summary(t["copy"], n_in, 16)}
        r["kernel"] = pfb.kernel
        r["xlat_kernel"] = xl[0].kernel
        r["taps_per_branch"] = -(-L // M)
        r["pfb_over_xlat_x_M"] = round(r["pfb"]["us"] / r["xlat_x_M"]["us"], 4)
        r["pfb_over_copy"] = round(r["pfb"]["us"] / r["copy"]["us"], 4)
        for p in xl:
            p.close()
        pfb.close()
        res["pfb"][f"M{M}_L{L}"] = r
        print(f"pfb M={M} L={L}:", json.dumps(r), flush=True)

    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
