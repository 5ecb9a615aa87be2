"""A/B of nsh_fft_filter_ccc across builds of libnsh_hip.so in one process on one stream: the first
path is the baseline (the parent commit's build), every other build is held against it.
Per (fft_size, ntaps) shape, on 2^LOG2N synthesized samples with a non-zero history:
  bits   out and hist_out of each build against the baseline's (bit-identical or not)
  time   ROUNDS interleaved rounds; in each, a build runs WARM untimed calls and then one call timed
         by its own event pair (nsh_time_next_launch); median, min and max per build. A build passes
         when its median is no higher than the baseline's slowest round.
Then two shapes of nsh_fft_xlat_ccc and one each of nsh_fft_c2c and nsh_psd_cf, bits only.
Exit status 1 if any output differs, 2 if only a time fails.
Usage: python tools/probe/ols_merge_ab.py PARENT.so NEW.so [MORE.so ...]
  env: LOG2N=26 ROUNDS=12 WARM=2 WARM_S=1 (seconds of all builds in turn before a shape's rounds)"""
import ctypes as C
import os
import sys
import time

import numpy as np
import scipy.signal as ss
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from newsched_amd.nsh import SIGNATURES  # noqa: E402  (the header's signatures; no library is loaded by this)

SHAPES = [(1024, 127), (2048, 512), (4096, 1024), (4096, 2048), (8192, 4096)]
paths = sys.argv[1:]
assert len(paths) >= 2, __doc__
libs = [C.CDLL(os.path.abspath(p), mode=C.RTLD_LOCAL) for p in paths]
for L in libs:
    for name, (res, args) in SIGNATURES.items():
        if name.startswith(("nsh_fft_", "nsh_psd_", "nsh_event_", "nsh_synth", "nsh_time_next", "nsh_last_error")):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
n = 1 << int(os.environ.get("LOG2N", "26"))
rounds = int(os.environ.get("ROUNDS", "12"))
warm = int(os.environ.get("WARM", "2"))
warm_s = float(os.environ.get("WARM_S", "1"))
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
bad_bits = bad_time = False


def ok(L, rc):
    assert rc == 0, L.nsh_last_error()


def synth(count, first):
    x = torch.empty(count, dtype=torch.complex64, device="cuda")
    ok(libs[0], libs[0].nsh_synth_cf32(x.data_ptr(), count, first, 0x6E736368, sp))
    s.synchronize()
    return x


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def same(a, b):
    return bool(torch.equal(torch.view_as_real(a).view(torch.int32), torch.view_as_real(b).view(torch.int32)))


def verdict(name, flags):
    global bad_bits
    bad_bits |= not all(flags)
    for p, f in zip(paths[1:], flags):
        print(f"  {name} {p}: {'bit-identical to' if f else 'DIFFERENT from'} {paths[0]}", flush=True)


x = synth(n, 0)
events = []
for L in libs:
    e = [C.c_void_p(), C.c_void_p()]
    for v in e:
        ok(L, L.nsh_event_create(C.byref(v)))
    events.append(e)
ys = [torch.zeros(n, dtype=torch.complex64, device="cuda") for _ in libs]

for N, ntaps in SHAPES:
    r = np.random.default_rng(N + ntaps)
    h = ((r.uniform(-1, 1, ntaps) + 1j * r.uniform(-1, 1, ntaps)) / ntaps).astype(np.complex64)
    hin = synth(ntaps - 1, 1 << 40)
    houts = [torch.zeros(ntaps - 1, dtype=torch.complex64, device="cuda") for _ in libs]
    plans, names = [], []
    for L in libs:
        p = C.c_void_p()
        ok(L, L.nsh_fft_filter_plan_create(0, fptr(h.view(np.float32)), ntaps, N, C.byref(p)))
        plans.append(p)
        names.append(L.nsh_fft_filter_kernel(p).decode())
    run = [lambda L=L, p=p, y=y, ho=ho: ok(L, L.nsh_fft_filter_ccc(p, x.data_ptr(), hin.data_ptr(), ho.data_ptr(), y.data_ptr(),
                                                                    n, sp)) for L, p, y, ho in zip(libs, plans, ys, houts)]
    for y in ys:
        y.zero_()
    torch.cuda.synchronize()  # the buffers were made on torch's stream
    for f in run:
        f()
    s.synchronize()
    print(f"fft_filter_ccc fft_size {N}, {ntaps} taps, 2^{n.bit_length() - 1} samples", flush=True)
    verdict("out", [same(ys[0], y) for y in ys[1:]])
    verdict("hist_out", [same(houts[0], ho) for ho in houts[1:]])
    t0 = time.perf_counter()  # clocks and power settle: every build in turn
    while time.perf_counter() - t0 < warm_s:
        for f in run:
            f()
        s.synchronize()
    t = [[] for _ in libs]
    for _ in range(rounds):
        for i, (L, f) in enumerate(zip(libs, run)):
            for _ in range(warm):
                f()
            ok(L, L.nsh_time_next_launch(events[i][0], events[i][1]))
            f()
            s.synchronize()
            ms = C.c_float()
            ok(L, L.nsh_event_elapsed_ms(events[i][0], events[i][1], C.byref(ms)))
            t[i].append(ms.value * 1e3)
    for i in range(len(libs)):
        v = sorted(t[i])
        line = f"  {paths[i]} {names[i]}: median {v[len(v) // 2]:.1f} us, min {v[0]:.1f}, max {v[-1]:.1f} over {rounds} rounds"
        if i:
            slower = v[len(v) // 2] > max(t[0])
            bad_time |= slower
            line += f"; median {'ABOVE' if slower else 'within'} the baseline's slowest round ({max(t[0]):.1f} us)"
        print(line, flush=True)
    for L, p in zip(libs, plans):
        L.nsh_fft_filter_plan_destroy(p)

# ---- the other entry points of the FFT family (their kernels' source is unchanged): bits only -----
m = min(n, 1 << 22)
h = (ss.firwin(127, 0.1) * np.exp(0.3j * np.arange(127))).astype(np.complex64)
hin = synth(126, 1 << 41)
for N, D in ((1024, 1), (2048, 8)):  # D = 1 tuned: the form next to fft_filter_ccc's; D > 1: the fold
    outs, houts = [], []
    for L in libs:
        p = C.c_void_p()
        ok(L, L.nsh_fft_xlat_plan_create(0, fptr(h.view(np.float32)), 127, D, 0.123, N, C.byref(p)))
        y = torch.zeros(m // D, dtype=torch.complex64, device="cuda")
        ho = torch.zeros(126, dtype=torch.complex64, device="cuda")
        torch.cuda.synchronize()
        ok(L, L.nsh_fft_xlat_ccc(p, x.data_ptr(), hin.data_ptr(), ho.data_ptr(), y.data_ptr(), m // D, 12345, sp))
        s.synchronize()
        name = L.nsh_fft_xlat_kernel(p).decode()
        L.nsh_fft_xlat_plan_destroy(p)
        outs.append(y)
        houts.append(ho)
    print(f"fft_xlat_ccc {name}, 127 taps, first_index 12345, {m} inputs", flush=True)
    verdict("out", [same(outs[0], y) for y in outs[1:]])
    verdict("hist_out", [same(houts[0], ho) for ho in houts[1:]])

win = np.hanning(4096).astype(np.float32)
outs = []
for L in libs:
    p = C.c_void_p()
    ok(L, L.nsh_fft_plan_create(0, 4096, 0, fptr(win), 1, C.byref(p)))
    y = torch.zeros(m, dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    ok(L, L.nsh_fft_c2c(p, x.data_ptr(), y.data_ptr(), m // 4096, sp))
    s.synchronize()
    name = L.nsh_fft_kernel(p).decode()
    L.nsh_fft_plan_destroy(p)
    outs.append(y)
print(f"fft_c2c {name}, window, shift, {m} samples", flush=True)
verdict("out", [same(outs[0], y) for y in outs[1:]])

win = np.hanning(1024).astype(np.float32)
outs = []
for L in libs:
    p = C.c_void_p()
    ok(L, L.nsh_psd_plan_create(0, 1024, 16, fptr(win), 1, 1.0 / 16, 0, C.byref(p)))
    y = torch.zeros(m // 16, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ok(L, L.nsh_psd_cf(p, x.data_ptr(), y.data_ptr(), m // 16 // 1024, sp))
    s.synchronize()
    name = L.nsh_psd_kernel(p).decode()
    L.nsh_psd_plan_destroy(p)
    outs.append(y)
print(f"psd_cf {name}, window, shift, 16 frames a vector, {m} samples", flush=True)
verdict("out", [bool(torch.equal(outs[0].view(torch.int32), y.view(torch.int32))) for y in outs[1:]])

print("bits: " + ("a build DIFFERS" if bad_bits else "all identical") + "; time: " +
      ("a median is ABOVE the baseline's slowest round" if bad_time else "every median within the baseline's spread"), flush=True)
sys.exit(1 if bad_bits else 2 if bad_time else 0)
