"""Kernel-level timing of the polyphase synthesis filterbank, every comparison interleaved in one
process. Each time is the kernel's own: an event pair armed with nsh_time_next_launch, recorded by the
launch itself.

  nsh_pfb_synthesizer_ccf   at (M, L) = (4, 31), (4, 127), (16, 127), (64, 127), (64, 511), 2^26 outputs
  nsh_pfb_channelizer_ccf   k_pfb<M> at the same (M, L) on 2^26 inputs: the same 16 B per wideband sample
  nsh_copy                  over the same 16 B per wideband sample (8 B read, 8 B written)
  substitute                what the existing blocks need for the same output: M nsh_resamp_ccf (I = M,
                            D = 1) launches on the channels' own streams, M nsh_rotate_cc and M - 1
                            nsh_add_cc (the sum of their 3 M - 1 kernel times; the split of the items
                            into M streams is not counted). --no-substitute leaves it out.

Per leg: a warm-up of at least 0.5 s of that leg, then the median over the rounds of the mean kernel
time of `reps` calls (us), the spread (min, max) of those rounds, wideband GS/s, and for the
filterbanks and the copy the fraction of 8 TB/s on 16 B per wideband sample. The legs alternate round
by round.

Usage: python tools/pfb_synth_bench.py [--rounds R] [--reps K] [--log2n N] [--out profiles/pfb_synth_bench.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from newsched_amd import nsh
from tools.pfb_bench import WARMUP_S, KernelTimer, interleaved, lowpass, summary

CASES = [(4, 31), (4, 127), (16, 127), (64, 127), (64, 511)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=26, help="wideband samples")
    ap.add_argument("--no-substitute", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "pfb_synth_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pfb_synth_bench needs a GPU"
    s = torch.cuda.Stream()
    n = 1 << a.log2n
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    y = torch.empty_like(x)
    nsh.synth(x, n, 0, stream=s)
    s.synchronize()
    timer = KernelTimer()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "warmup_s": WARMUP_S,
           "n_wideband": n, "timing": "kernel time from the launch's own event pair (nsh_time_next_launch)", "synth": {}}
    if not a.no_substitute:
        acc = torch.empty_like(x)

    for M, L in CASES:
        taps = lowpass(L, M)
        items = n // M
        H = (-(-L // M) - 1) * M
        syn = nsh.PfbSynthPlan(taps, M)
        pfb = nsh.PfbPlan(taps, M)
        hin = torch.zeros(max(L - 1, 1), dtype=torch.complex64, device="cuda")
        hout = torch.zeros_like(hin)
        assert H <= L - 1
        legs = {
            "synth": [lambda: syn(x, hin, hout, y, items, stream=s)],
            "pfb": [lambda: pfb(x, hin, hout, y, items, stream=s)],
            "copy": [lambda: nsh.copy(x, y, 8 * n, stream=s)],
        }
        if not a.no_substitute:
            rs = nsh.ResampPlan(taps, M, 1)
            sub = []
            for c in range(M):      # channel c's own stream: items samples of x
                xc = x[c * items:(c + 1) * items]
                out = acc if c == 0 else y
                sub.append(lambda xc=xc, out=out: rs(xc, hin, hout, out, items, stream=s))
                sub.append(lambda c=c, out=out: nsh.rotate_cc(out, out, n, nsh.phase_inc(c / M), 0, stream=s))
                if c:
                    sub.append(lambda: nsh.add_cc(acc, y, acc, n, stream=s))
            assert len(sub) == 3 * M - 1
            legs["substitute"] = sub
        t = interleaved(legs, a.rounds, a.reps, timer)
        r = {k: summary(t[k], n, None if k == "substitute" else 16) for k in legs}
        r["kernel"] = syn.kernel
        r["taps_per_branch"] = -(-L // M)
        r["synth_over_copy"] = round(r["synth"]["us"] / r["copy"]["us"], 4)
        r["synth_over_pfb"] = round(r["synth"]["us"] / r["pfb"]["us"], 4)
        r["pfb_over_copy"] = round(r["pfb"]["us"] / r["copy"]["us"], 4)
        if not a.no_substitute:
            r["substitute_launches"] = 3 * M - 1
            r["substitute_over_synth"] = round(r["substitute"]["us"] / r["synth"]["us"], 2)
            rs.close()
        syn.close()
        pfb.close()
        res["synth"][f"M{M}_L{L}"] = r
        print(f"synth M={M} L={L}:", json.dumps(r), flush=True)

    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
