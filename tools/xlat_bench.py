"""Kernel-level timing of the rotator and the frequency-translating FIR (HIP events on the launch
stream), every comparison interleaved in one process:

  nsh_rotate_cc      against nsh_mul_const_cc (same bytes: 16 B per sample) at 2^26 .. 2^28 samples
  nsh_fir_xlat_ccf   at (D, L) = (1, 127), (2, 127), (4, 127), (8, 127), (16, 127), (16, 255), (64, 1024)
                     against the staged nsh_rotate_cc -> nsh_fir_ccf(AUTO) where nsh_fir_ccf has the
                     decimation (1, 2, 4, 8, 16)

Per leg: the median over the rounds of the mean time of `reps` back-to-back calls (us), the spread
(min, max) of those rounds, input GS/s, and the fraction of 8 TB/s on the algorithmic bytes (16 B per
sample for the rotator, 8 + 8/D B per input for the translating FIR, staged or fused). The legs of
one comparison alternate round by round, after a warm-up of every leg.

Usage: python tools/xlat_bench.py [--rounds R] [--reps K] [--log2n N] [--out profiles/xlat_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from newsched_amd import nsh

HBM_BPS = 8e12
CASES = [(1, 127), (2, 127), (4, 127), (8, 127), (16, 127), (16, 255), (64, 1024)]


def window_us(fn, reps, stream):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        st.record(stream)
        for _ in range(reps):
            fn()
        en.record(stream)
    en.synchronize()
    return 1e3 * st.elapsed_time(en) / reps


def interleaved(legs, rounds, reps, stream):
    """legs: {name: fn}. Returns {name: [us per round]}, the legs alternating within each round."""
    for fn in legs.values():  # warm-up: code objects, plan queues, clocks
        window_us(fn, 3, stream)
    out = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            out[k].append(window_us(fn, reps, stream))
    return out


def summary(us, n_in, bytes_per_in):
    med = statistics.median(us)
    return {"us": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
            "spread": round((max(us) - min(us)) / med, 4), "GS/s_in": round(n_in / med / 1e3, 2),
            "hbm_frac": round(bytes_per_in * n_in / (med * 1e-6) / HBM_BPS, 4)}


def lowpass(L, D):
    k = np.arange(L) - (L - 1) / 2.0
    t = np.hamming(L) * np.sinc(0.8 * k / D)
    return (t / t.sum()).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2n", type=int, default=26, help="inputs of the FIR legs")
    ap.add_argument("--out", default=os.path.join("profiles", "xlat_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "xlat_bench needs a GPU"
    s = torch.cuda.Stream()
    nmax = 1 << 28
    x = torch.empty(nmax, dtype=torch.complex64, device="cuda")
    y = torch.empty_like(x)
    nsh.synth(x, nmax, 0, stream=s)
    s.synchronize()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "rotator": {}, "xlat": {}}

    inc = nsh.phase_inc(0.1234)
    for lg in (26, 27, 28):
        n = 1 << lg
        t = interleaved({"rotate_cc": lambda: nsh.rotate_cc(x, y, n, inc, 12345, stream=s),
                         "mul_const_cc": lambda: nsh.mul_const_cc(x, y, n, complex(np.exp(0.3j)), stream=s),
                         "mul_const_cc_again": lambda: nsh.mul_const_cc(x, y, n, complex(np.exp(0.3j)), stream=s)},
                        a.rounds, a.reps, s)
        r = {k: summary(v, n, 16) for k, v in t.items()}
        r["rotate_over_mul_const"] = round(r["rotate_cc"]["us"] / r["mul_const_cc"]["us"], 4)
        # the run-to-run spread of mul_const_cc itself: its two interleaved legs' medians, and the rounds of one
        r["mul_const_self_ratio"] = round(r["mul_const_cc_again"]["us"] / r["mul_const_cc"]["us"], 4)
        res["rotator"][f"2^{lg}"] = r
        print(f"rotator 2^{lg}:", json.dumps(r), flush=True)

    n_in = 1 << a.log2n
    for D, L in CASES:
        taps = lowpass(L, D)
        n_out = n_in // D
        fused = nsh.FirXlatPlan(taps, D, 0.1234)
        hin = torch.zeros(max(L - 1, 1), dtype=torch.complex64, device="cuda")
        hout = torch.zeros_like(hin)
        legs = {"fused": lambda: fused(x, hin, hout, y, n_out, 12345, stream=s)}
        staged = None
        if D in (1, 2, 4, 8, 16):
            staged = nsh.FirPlan(taps, D, nsh.FIR_AUTO)
            tmp = torch.empty(n_in, dtype=torch.complex64, device="cuda")

            def run_staged():
                nsh.rotate_cc(x, tmp, n_in, fused.inc, 12345, stream=s)
                staged(tmp, hin, hout, y, n_out, stream=s)

            legs["staged"] = run_staged
        t = interleaved(legs, a.rounds, a.reps, s)
        r = {k: summary(v, n_in, 8 + 8 / D) for k, v in t.items()}
        r["kernel"] = fused.kernel
        r["fma_per_input"] = round(2 * L / D, 2)
        if staged is not None:
            r["staged_kernel"] = "k_rotate + " + staged.kernel
            r["fused_over_staged"] = round(r["fused"]["us"] / r["staged"]["us"], 4)
            staged.close()
        fused.close()
        res["xlat"][f"D{D}_L{L}"] = r
        print(f"xlat D={D} L={L}:", json.dumps(r), flush=True)

    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
