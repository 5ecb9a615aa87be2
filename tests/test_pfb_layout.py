"""k_pfb<M>'s LDS images and work mapping, checked on the host (CPU only) for every instantiation:
the geometry of nsh_pfb.hip's geom<M> (restated here), the bank model of tests/test_lds_layouts.py
for the branch FIR's per-lane ds_read_b64 and the store image's ds_write_b64, an index-level walk of
the kernel's loops (every (time step, tap) pair is met exactly once with the right stream sample, no
tap at or past L is touched, no LDS entry past the allocation is used, every output sample is
stored once), and the radix-2 lane-exchange network against numpy's inverse DFT."""
import numpy as np
import pytest

from tests.test_lds_layouts import B64, cycles

KBLOCK, R, QC = 256, 8, 4
MS = [2, 4, 8, 16, 32, 64]
W64 = [list(range(16 * g, 16 * g + 16)) for g in range(4)]   # ds_write_b64: 4 groups of 16 contiguous lanes


class Geom:
    """geom<M> of nsh_pfb.hip."""

    def __init__(self, M):
        self.M, self.log2m = M, M.bit_length() - 1
        self.G = KBLOCK // M
        self.T = self.G * R
        self.rounds = 2
        self.RH = R // self.rounds
        self.YW = 64 * self.RH + 64

    def row_entry(self, j):
        return (j + (j >> 3) if self.M < 32 else j) * self.M

    def ypos(self, e):
        if self.M >= 32:
            return e + (e >> 4)
        return e + ((e >> ((self.RH.bit_length() - 1) + self.log2m)) << self.log2m)

    def lds_bytes(self, L):
        Q = -(-L // self.M)
        Qp = -(-Q // QC) * QC
        return self.row_entry(self.T + Q - 1) * 8 + Qp * self.M * 4 + (KBLOCK // 64) * self.YW * 8


def bitrev(p, bits):
    return int(format(p, f"0{bits}b")[::-1], 2) if bits else 0


@pytest.mark.parametrize("M", MS)
def test_tile_and_lds_budget(M):
    g = Geom(M)
    assert g.T * M == 2048
    assert g.lds_bytes(32 * M if 32 * M <= 1024 else 1024) <= 160 * 1024
    assert (160 * 1024) // g.lds_bytes(8 * M - 1) >= 5   # workgroups per CU at Q = 8


@pytest.mark.parametrize("M", MS)
def test_branch_reads_conflict_free(M):
    g = Geom(M)
    for Q in (1, 8, 32):
        if Q * M > 1024 and (Q - 1) * M >= 1024:
            continue
        for wave in range(4):
            for rho in (0, 1, 5, R + Q - 2):              # any row of the lanes' windows: the same rho in every lane
                addr = []
                for lane in range(64):
                    tid = wave * 64 + lane
                    p, tg = tid % M, tid // M
                    addr.append(8 * (g.row_entry(tg * R + rho) + (M - 1 - p)))
                assert cycles(addr, B64, 8) == 2, (M, Q, wave, rho)


@pytest.mark.parametrize("M", [2, 4, 8, 16])
def test_packed_rows_would_conflict(M):
    """why rows are not packed at M < 32: time groups R rows apart share their banks"""
    addr = [8 * (((lane // M) * R) * M + (M - 1 - lane % M)) for lane in range(64)]
    assert cycles(addr, B64, 8) >= 4                    # 2 when conflict-free


@pytest.mark.parametrize("M", MS)
def test_store_image_writes_conflict_free_and_reads_linear(M):
    g = Geom(M)
    ch = [bitrev(lane % M, g.log2m) for lane in range(64)]
    used = set()
    for t in range(g.RH):
        addr = [8 * g.ypos((((lane // M) * g.RH + t) << g.log2m) + ch[lane]) for lane in range(64)]
        assert cycles(addr, W64, 8, nbank=32) == 4, (M, t)
        used |= {a // 8 for a in addr}
    assert len(used) == 64 * g.RH and max(used) < g.YW     # a permutation of the round's samples, inside the image
    for e in range(0, 64 * g.RH, 2):                        # a pair is two neighbouring entries of one time step
        assert g.ypos(e + 1) == g.ypos(e) + 1
        assert (e % (g.RH * M)) // M == ((e + 1) % (g.RH * M)) // M


@pytest.mark.parametrize("M,L", [(2, 1), (2, 64), (4, 48), (8, 127), (16, 16), (16, 127), (32, 385), (64, 65), (64, 1024),
                                 (64, 200), (32, 1024)])
def test_walk_meets_every_tap_once(M, L):
    g = Geom(M)
    Q = -(-L // M)
    Qp = -(-Q // QC) * QC
    rows = g.T + Q - 1
    window_entries = g.row_entry(rows)
    for tid in (0, 1, M - 1, M, KBLOCK // 2 + 3, KBLOCK - 1):
        p, tg = tid % M, tid // M
        qv, qall = (L - p + M - 1) >> g.log2m, L >> g.log2m
        col = M - 1 - p
        trow = tg * R
        met = {}

        def row(rho):
            j = trow + max(rho, 0)
            assert j < rows and g.row_entry(j) + col < window_entries
            return j * M + col                          # the window position that entry holds

        lo = Q - QC
        xw = [row(lo + k) for k in range(R + QC - 1)]
        nreads = R + QC - 1
        for q0 in range(0, Qp, QC):
            for dq in range(QC):
                q = q0 + dq
                if q0 + QC <= qall or q < qv:           # the fast path, or the per-lane test
                    assert p + q * M < L
                    for t in range(R):
                        assert (t, q) not in met
                        met[(t, q)] = xw[t + QC - 1 - dq]
            if q0 + QC < Qp:
                lo -= QC
                xw = [row(lo + k) for k in range(QC)] + xw[:R - 1]
                nreads += QC
        assert nreads == R + Qp - 1
        assert len(met) == R * len([q for q in range(Q) if p + q * M < L])
        for (t, q), w in met.items():
            # window position 0 is stream sample (m0 - (Q-1)) M - (M-1); x[(m - q) M - p], m = m0 + trow + t
            assert w == (trow + t - q + Q - 1) * M - p + (M - 1)


@pytest.mark.parametrize("M", MS)
def test_every_output_stored_once(M):
    g = Geom(M)
    for vec in (True, False):
        seen = {}
        for wave in range(4):
            mw = wave * (64 // M) * R
            for rd in range(g.rounds):
                image = {}
                for lane in range(64):
                    p, tgl = lane % M, lane // M
                    for t in range(g.RH):
                        e = ((tgl * g.RH + t) << g.log2m) + bitrev(p, g.log2m)
                        image[g.ypos(e)] = (mw + tgl * R + rd * g.RH + t, bitrev(p, g.log2m))
                step = 2 if vec else 1
                for i in range(g.RH // step):
                    for lane in range(64):
                        e = step * (64 * i + lane)
                        blk, rest = e // (g.RH * M), e % (g.RH * M)
                        m, c = mw + blk * R + rd * g.RH + rest // M, rest % M
                        for k in range(step):
                            assert image[g.ypos(e) + k] == (m, c + k)
                            assert (m, c + k) not in seen
                            seen[(m, c + k)] = True
        assert len(seen) == g.T * M and all(0 <= m < g.T for m, _ in seen)


def twiddles(M):
    """the table nsh_pfb_plan_create uploads: tw[s][lane], float32 of double values"""
    stages = M.bit_length() - 1
    tw = np.ones((max(stages - 1, 0), M), np.complex64)
    for s in range(stages - 1):
        half = M >> (s + 1)
        for q in range(M):
            if q & half:
                i = q & (half - 1)
                v = np.exp(2j * np.pi * i / (2 * half))
                if 4 * i == 2 * half:
                    v = 1j
                tw[s, q] = np.complex64(v)
    return tw


@pytest.mark.parametrize("M", MS)
def test_lane_exchange_network_is_the_inverse_dft(M):
    stages = M.bit_length() - 1
    rng = np.random.default_rng(M)
    u = (rng.standard_normal(M) + 1j * rng.standard_normal(M)).astype(np.complex64)
    tw = twiddles(M)
    a = u.copy()
    lanes = np.arange(M)
    for s in range(stages):
        half = M >> (s + 1)
        b = a[lanes ^ half]
        sgn = np.where(lanes & half, -1.0, 1.0).astype(np.float32)
        t = (a * sgn + b).astype(np.complex64)
        a = (t * tw[s]).astype(np.complex64) if s < stages - 1 else t
    y = np.empty(M, np.complex64)
    for p in range(M):
        y[bitrev(p, stages)] = a[p]
    ref = np.fft.ifft(u.astype(np.complex128)) * M
    assert np.max(np.abs(y - ref)) <= 1e-6 * np.max(np.abs(ref))
