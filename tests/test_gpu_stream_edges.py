"""GPU: the stream kernels of nsh_stream.hip (multiply_const cc / ff / chain / vcc, add_cc,
multiply_cc, synth) at the values and pointers test_gpu_kernels.py leaves out: signed zeros,
subnormal operands and products, overflow to inf, inf - inf, NaN; 4- and 8-byte aligned pointers and
the tail launches; chain lengths 0, 5..16 and 17; synth indices at and beyond 2^31 and at the 2^64 wrap.

Everything is bit-exact against the oracle ("same formula, no FMA": a flushed subnormal or a fused
multiply-add shows as a bit difference). Where the oracle's output is NaN only the NaN's position is
compared; signed zeros and infinities are compared bitwise."""
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle import oracle as orc
from newsched_amd import nsh
from tests.gpu_util import dev, host

pytestmark = pytest.mark.gpu

GUARD = complex(9.0, -9.0)
FLT_MAX = float(np.finfo(np.float32).max)
TINY = float(np.float32(1e-45))  # the smallest subnormal, 2^-149


def assert_bits(y, r, what=""):
    """y == r bit for bit, except where r is NaN: there y must be NaN too (any payload)."""
    yf = np.ascontiguousarray(y).view(np.float32).ravel()
    rf = np.ascontiguousarray(r).view(np.float32).ravel()
    assert yf.size == rf.size, what
    nan = np.isnan(rf)
    np.testing.assert_array_equal(np.isnan(yf), nan, err_msg=what + ": NaN positions")
    bad = np.nonzero(yf.view(np.uint32)[~nan] != rf.view(np.uint32)[~nan])[0]
    assert bad.size == 0, (what, bad.size, bad[:6].tolist(), yf[~nan][bad[:6]].tolist(), rf[~nan][bad[:6]].tolist())


# fp32 parts: signed zeros, subnormals, factors of subnormal products (1e-30 x 1e-10), of overflowing
# products (1e30 x 1e30, FLT_MAX x 2), ordinary values with full mantissas (a fused multiply-add
# rounds their a b - c d differently), +-inf and NaN
PARTS = np.array([0.0, -0.0, 1e-40, -1e-40, TINY, 1e-30, 1e-10, 1e30, -1e30, FLT_MAX, 2.0, 1.0, -1.0, 0.5,
                  1.1, -0.7, np.inf, -np.inf, np.nan], np.float32)
assert PARTS[4] > 0 and PARTS[2] < np.finfo(np.float32).tiny  # subnormals survived the conversion


def table():
    """Every (re, im) pair of PARTS: 361 complex operands; holds (inf, 1) and (1, inf), whose
    product is inf - inf in the real part."""
    re, im = np.meshgrid(PARTS, PARTS, indexing="ij")
    t = np.empty(re.size, np.complex64)
    t.real, t.imag = re.ravel(), im.ravel()
    return t


def pair_table():
    """Every ordered pair of table() operands (130321 pairs, an odd count)."""
    t = table()
    return np.repeat(t, t.size), np.tile(t, t.size)


def lengths(v):
    """v at an even and an odd length, so both the 16-byte kernel and the launch for an odd tail run
    (two passes of v: each value meets both halves of a 16-byte lane; the odd one ends one early)."""
    vv = np.concatenate([v, v[:-1]] if v.size % 2 else [v[1:], v])
    assert vv.size % 2 == 1
    return [np.concatenate([vv, v[:1]]), vv]


def placed(torch, v, off):
    """v on the device at a sample offset into a zeroed allocation; returns (tensor, address)."""
    d = torch.zeros(v.size + 2, dtype=torch.complex64, device="cuda")
    d[off:off + v.size] = dev(torch, v)
    return d, d.data_ptr() + 8 * off


def guarded_out(torch, n, off):
    d = torch.full((n + 4,), GUARD, dtype=torch.complex64, device="cuda")
    return d, d.data_ptr() + 8 * off


def result(dy, n, off):
    y = host(dy)
    g = np.complex64(GUARD)
    assert np.all(y[:off] == g) and np.all(y[off + n:] == g), "guard samples overwritten"
    return y[off:off + n]


CONSTS = [complex(1e-10, 1e30), complex(np.inf, 1.0), complex(1.0, np.inf), complex(-0.0, 0.0), complex(np.nan, 1.0),
          complex(1e-40, 2.0), complex(FLT_MAX, 1.1), complex(0.7, -1.1), complex(1e30, -1e-30), complex(TINY, -0.5)]


@pytest.mark.parametrize("off", [0, 1], ids=["aligned16", "plus8bytes"])
def test_mul_const_cc_edge_values(torch_cuda, off):
    torch = torch_cuda
    for v in lengths(table()):
        dx, px = placed(torch, v, off)
        for k in CONSTS:
            dy, py = guarded_out(torch, v.size, 2 + off)
            nsh.mul_const_cc(px, py, v.size, k)
            assert_bits(result(dy, v.size, 2 + off), orc.mul_const_cc(v, k), "k=%r n=%d" % (k, v.size))


@pytest.mark.parametrize("off", [0, 1], ids=["aligned16", "plus8bytes"])
def test_mul_add_cc_edge_values(torch_cuda, off):
    """Every ordered pair of the operand table through multiply_cc and add_cc."""
    torch = torch_cuda
    a, b = pair_table()
    for va, vb in zip(lengths(a), lengths(b)):
        n = va.size
        (da, pa), (db, pb) = placed(torch, va, off), placed(torch, vb, off)
        for fn, oracle in ((nsh.mul_cc, orc.mul_cc), (nsh.add_cc, orc.add_cc)):
            dy, py = guarded_out(torch, n, 2 + off)
            fn(pa, pb, py, n)
            assert_bits(result(dy, n, 2 + off), oracle(va, vb), "%s n=%d" % (oracle.__name__, n))


CHAINS = [[complex(1e-20, 0.0), complex(1e-20, 1e-20), complex(1e30, 0.0), complex(1e10, -1e10)],
          [complex(2.0, 0.0), complex(0.5, 0.5), complex(1e30, 1e30), complex(1e-30, -0.0)],
          [complex(1.1, -0.7), complex(-0.7, 1.1), complex(1e-10, 1e-10), complex(1e-30, 1.0)]]


@pytest.mark.parametrize("off", [0, 1], ids=["aligned16", "plus8bytes"])
def test_mul_const_chain4_edge_values(torch_cuda, off):
    """The 4-stage chain (C2's kernel, op_chain<4>): each stage rounds, so intermediate subnormals,
    infinities and NaNs must appear and vanish exactly where the oracle's do."""
    torch = torch_cuda
    for v in lengths(table()):
        dx, px = placed(torch, v, off)
        for ks in CHAINS:
            dy, py = guarded_out(torch, v.size, 2 + off)
            nsh.mul_const_chain_cc(px, py, v.size, ks)
            assert_bits(result(dy, v.size, 2 + off), orc.mul_const_chain_cc(v, ks), "ks=%r n=%d" % (ks, v.size))


FCONSTS = [1e-10, 1e30, 2.0, -0.0, 0.5, 1.1, float("inf"), float("nan"), 1e-40, TINY]


def fdev(torch, v, byte_off):
    """float32 v on the device at a byte offset (multiple of 4) into a zeroed allocation."""
    d = torch.zeros(v.size + 8, dtype=torch.float32, device="cuda")
    d[byte_off // 4:byte_off // 4 + v.size] = dev(torch, v)
    return d, d.data_ptr() + byte_off


def fresult(torch, px, n, k, byte_off):
    d = torch.full((n + 8,), 7.5, dtype=torch.float32, device="cuda")
    nsh.mul_const_ff(px, d.data_ptr() + byte_off, n, k)
    y = host(d)
    o = byte_off // 4
    assert np.all(y[:o] == 7.5) and np.all(y[o + n:] == 7.5), "guard floats overwritten"
    return y[o:o + n]


def test_mul_const_ff_edge_values(torch_cuda):
    """Every part value times every constant, at lengths 4 k .. 4 k + 3 (the 16-byte kernel plus each
    tail launch) and at a 4-byte aligned pointer (the scalar kernel)."""
    torch = torch_cuda
    base = np.tile(PARTS, 4)[:72]
    for extra, off in itertools.product(range(4), (0, 4)):
        v = np.concatenate([base, PARTS[:extra]])
        dx, px = fdev(torch, v, off)
        for k in FCONSTS:
            assert_bits(fresult(torch, px, v.size, k, off), orc.mul_const_ff(v, k), "k=%r n=%d off=%d" % (k, v.size, off))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1023, 1024, 1025])
def test_mul_const_ff_lengths_and_alignments(torch_cuda, n):
    """Byte offsets 0, 4, 8, 12 of either pointer: the 16-byte kernel with its n % 4 tail launch when
    both are 16-byte aligned, the scalar kernel otherwise; guards on both sides of the output."""
    torch = torch_cuda
    v = orc.synth(n, 17).view(np.float32)[:n].copy()
    r = orc.mul_const_ff(v, 1.7)
    for in_off, out_off in itertools.product((0, 4, 8, 12), repeat=2):
        dx, px = fdev(torch, v, in_off)
        d = torch.full((n + 8,), 7.5, dtype=torch.float32, device="cuda")
        nsh.mul_const_ff(px, d.data_ptr() + 16 + out_off, n, 1.7)
        y = host(d)
        o = 4 + out_off // 4
        np.testing.assert_array_equal(y[o:o + n].view(np.uint32), r.view(np.uint32), err_msg=str((in_off, out_off)))
        assert np.all(y[:o] == 7.5) and np.all(y[o + n:] == 7.5), (in_off, out_off)


@pytest.mark.parametrize("n", [1, 2, 1001, 4096])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned16", "plus8bytes"])
def test_mul_const_chain_zero_stages_is_a_copy(torch_cuda, n, off):
    """m = 0 moves the samples unchanged (nsh_copy): every bit, NaN payloads and signed zeros included."""
    torch = torch_cuda
    v = np.resize(table(), n)
    v.view(np.uint32)[-1] = 0x7FC01234  # a NaN with a payload in the last part
    dx, px = placed(torch, v, off)
    dy, py = guarded_out(torch, n, 2 + off)
    nsh.mul_const_chain_cc(px, py, n, [])
    np.testing.assert_array_equal(result(dy, n, 2 + off).view(np.uint32), v.view(np.uint32))


@pytest.mark.parametrize("m", [5, 8, 16])
def test_mul_const_chain_dynamic_lengths(torch_cuda, m):
    """The dynamic-length kernel (op_chain_dyn, any m without an instantiation of its own) up to its
    limit of 16 stages, odd n, aligned and at +8 bytes."""
    torch = torch_cuda
    n = 4097
    x = orc.synth(n, 19)
    ks = [complex(np.exp(0.1j * (i + 1))) * (1.0 + 0.01 * i) for i in range(m)]
    r = orc.mul_const_chain_cc(x, [np.complex64(k) for k in ks])
    for off in (0, 1):
        dx, px = placed(torch, x, off)
        dy, py = guarded_out(torch, n, 2 + off)
        nsh.mul_const_chain_cc(px, py, n, ks)
        np.testing.assert_array_equal(result(dy, n, 2 + off).view(np.uint32), r.view(np.uint32))


def test_mul_const_chain_refuses_17_stages(torch_cuda):
    torch = torch_cuda
    n = 1000
    dx, px = placed(torch, orc.synth(n, 19), 0)
    dy, py = guarded_out(torch, n, 2)
    with pytest.raises(nsh.NshError, match="at most 16 fused stages"):
        nsh.mul_const_chain_cc(px, py, n, [1.0 + 0.5j] * 17)
    assert np.all(host(dy) == np.complex64(GUARD))


@pytest.mark.parametrize("vlen,nitems", [(1024, 1027), (1000, 1051), (7, 149_801)])
def test_mul_const_vcc_odd_offsets_past_one_sweep(torch_cuda, vlen, nitems):
    """in, out and k each at +8 bytes; more than 2^20 samples, so the 4096-workgroup grid walks a
    second, partial sweep (ending inside a workgroup for vlen 1000 and 7); the kernel indexes k by the
    sample's position modulo vlen."""
    torch = torch_cuda
    n = vlen * nitems
    assert (1 << 20) < n < (1 << 21)
    x = orc.synth(n, 91)
    k = orc.synth(vlen, 92)
    dx, px = placed(torch, x, 1)
    dk, pk = placed(torch, k, 1)
    dy, py = guarded_out(torch, n, 1)
    nsh.mul_const_vcc(px, py, pk, vlen, nitems)
    np.testing.assert_array_equal(result(dy, n, 1).view(np.uint32), orc.mul_cc(x, np.tile(k, nitems)).view(np.uint32))


@pytest.mark.parametrize("first", [2 ** 31 - 3, 2 ** 32 - 3, 2 ** 40 + 1, 2 ** 63 - 2, 2 ** 64 - 5],
                         ids=["2^31-3", "2^32-3", "2^40+1", "2^63-2", "2^64-5"])
def test_synth_large_first_index(torch_cuda, first):
    """g = 2 (first + i) in 64 bits, wrapping at 2^64 as the oracle does: a 32-bit truncation
    anywhere in the index shows from 2^31 on. first_index is passed as a Python int (c_uint64)."""
    torch = torch_cuda
    assert nsh.SIGNATURES["nsh_synth_cf32"][1][2] is C.c_uint64 and nsh.SIGNATURES["nsh_synth_cf32"][1][3] is C.c_uint64
    n = 4097
    y = torch.full((n + 2,), GUARD, dtype=torch.complex64, device="cuda")
    nsh.synth(y.data_ptr() + 8, n, first)
    got = host(y)
    np.testing.assert_array_equal(got[1:1 + n].view(np.uint32), orc.synth(n, first).view(np.uint32))
    assert got[0] == np.complex64(GUARD) and got[-1] == np.complex64(GUARD)


def test_synth_other_seed(torch_cuda):
    torch = torch_cuda
    n = 4097
    y = torch.empty(n, dtype=torch.complex64, device="cuda")
    for first, seed in ((0, 0x1234567), (2 ** 64 - 5, 2 ** 64 - 1), (2 ** 40 + 1, 0)):
        nsh.synth(y, n, first, seed)
        np.testing.assert_array_equal(host(y).view(np.uint32), orc.synth(n, first, seed).view(np.uint32))
    assert not np.array_equal(orc.synth(n, 0, 0x1234567), orc.synth(n, 0))
