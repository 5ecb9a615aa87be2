"""k_pfb_synth<M>'s LDS images and work mapping, checked on the host (CPU only) for every
instantiation. The tile geometry, the row pitch, the FIR walk and the store image are k_pfb's geom<M>
(tests/test_pfb_layout.py, whose Geom and transform model this file uses). What differs is restated
here: the window is written one transformed item per M lanes at column bitrev(lane), columns are
xor-swizzled at M >= 32 (col_entry), the FIR reads column r, and the store image is written at
channel r. Bank model of tests/test_lds_layouts.py."""
import numpy as np
import pytest

from tests.test_lds_layouts import B64, cycles
from tests.test_pfb_layout import KBLOCK, MS, QC, R, W64, Geom, bitrev, twiddles

KSTAGE, KTAIL = 8, 2


def col_entry(M, c):
    """col_entry<M> of nsh_pfb_synth.hip."""
    return c ^ ((c >> 4) & (M // 16 - 1)) if M >= 32 else c


def passes(count):
    """(first window position, items per lane) of the staging passes."""
    out = [(0, KSTAGE)]
    b = KBLOCK * KSTAGE
    while b < count:
        out.append((b, KTAIL))
        b += KBLOCK * KTAIL
    return out


@pytest.mark.parametrize("M", MS)
def test_col_entry_is_a_permutation_inside_aligned_groups(M):
    cols = [col_entry(M, c) for c in range(M)]
    assert sorted(cols) == list(range(M))
    grp = max(M // 16, 1)
    assert all(cols[c] // grp == c // grp for c in range(M))     # 32 consecutive columns stay 32 consecutive entries


@pytest.mark.parametrize("M,L", [(2, 1), (2, 64), (4, 48), (8, 127), (16, 16), (16, 127), (32, 385), (32, 1024), (64, 65),
                                 (64, 200), (64, 1024)])
def test_staging_fills_every_window_entry_once_without_conflicts(M, L):
    g = Geom(M)
    Q = -(-L // M)
    rows = g.T + Q - 1
    count = rows * M
    filled = {}
    for b, n in passes(count):
        for u in range(n):
            for wave in range(KBLOCK // 64):
                addr, live = [], []
                for lane in range(64):
                    tid = wave * 64 + lane
                    i = b + KBLOCK * u + tid
                    p = tid % M
                    assert i % M == p                              # a lane keeps its channel
                    e = g.row_entry(i // M) + col_entry(M, bitrev(p, g.log2m))
                    addr.append(8 * e)
                    live.append(i < count)
                    if i < count:
                        assert e not in filled and e < g.row_entry(rows)
                        filled[e] = (i // M, bitrev(p, g.log2m))       # (row, branch r) the entry holds
                # the M lanes of an item are in or out together (the lane exchange needs all of them)
                for k in range(0, 64, M):
                    assert len(set(live[k:k + M])) == 1
                if all(live):
                    assert cycles(addr, W64, 8, nbank=32) == 4, (M, b, u, wave)
    assert len(filled) == count
    assert sum(n for _, n in passes(count)) * KBLOCK >= count
    # the FIR's column r of row j is where the staging put branch r of that row
    for j in (0, 7, 8, rows - 1):
        for r in range(M):
            assert filled[g.row_entry(j) + col_entry(M, r)] == (j, r)


@pytest.mark.parametrize("M", [32, 64])
def test_unswizzled_bitreversed_writes_would_conflict(M):
    g = Geom(M)
    addr = [8 * (g.row_entry(lane // M) + bitrev(lane % M, g.log2m)) for lane in range(64)]
    assert cycles(addr, W64, 8, nbank=32) == 4 * (M // 16)


@pytest.mark.parametrize("M", MS)
def test_branch_reads_conflict_free(M):
    g = Geom(M)
    for wave in range(4):
        for rho in (0, 1, 5, R + 30):
            addr = []
            for lane in range(64):
                tid = wave * 64 + lane
                r, tg = tid % M, tid // M
                addr.append(8 * (g.row_entry(tg * R + rho) + col_entry(M, r)))
            assert cycles(addr, B64, 8) == 2, (M, wave, rho)


@pytest.mark.parametrize("M,L", [(2, 1), (2, 64), (4, 48), (8, 127), (16, 127), (32, 385), (64, 65), (64, 1024), (32, 1024)])
def test_walk_meets_every_tap_once(M, L):
    """k_pfb's walk at column r: output (m0 + trow + t) M + r meets h[r + q M] v_r[m - q], no tap at or past L."""
    g = Geom(M)
    Q = -(-L // M)
    Qp = -(-Q // QC) * QC
    rows = g.T + Q - 1
    for tid in (0, 1, M - 1, M, KBLOCK // 2 + 3, KBLOCK - 1):
        r, tg = tid % M, tid // M
        qv, qall = (L - r + M - 1) >> g.log2m, L >> g.log2m
        trow = tg * R
        met = {}

        def row(rho):
            j = trow + max(rho, 0)
            assert j < rows
            return j

        lo = Q - QC
        xw = [row(lo + k) for k in range(R + QC - 1)]
        for q0 in range(0, Qp, QC):
            for dq in range(QC):
                q = q0 + dq
                if q0 + QC <= qall or q < qv:
                    assert r + q * M < L
                    for t in range(R):
                        assert (t, q) not in met
                        met[(t, q)] = xw[t + QC - 1 - dq]
            if q0 + QC < Qp:
                lo -= QC
                xw = [row(lo + k) for k in range(QC)] + xw[:R - 1]
        assert len(met) == R * len([q for q in range(Q) if r + q * M < L])
        for (t, q), j in met.items():
            assert j == trow + t - q + Q - 1          # window row 0 is item m0 - (Q-1)


@pytest.mark.parametrize("M", MS)
def test_store_image_writes_conflict_free_and_outputs_stored_once(M):
    g = Geom(M)
    for vec in (True, False):
        seen = set()
        for wave in range(4):
            mw = wave * (64 // M) * R
            for rd in range(g.rounds):
                image = {}
                for t in range(g.RH):
                    addr = [8 * g.ypos((((lane // M) * g.RH + t) << g.log2m) + lane % M) for lane in range(64)]
                    assert cycles(addr, W64, 8, nbank=32) == 4, (M, t)
                    for lane in range(64):
                        image[addr[lane] // 8] = ((mw + (lane // M) * R + rd * g.RH + t) * M + lane % M)
                assert len(image) == 64 * g.RH and max(image) < g.YW
                step = 2 if vec else 1
                for i in range(g.RH // step):
                    for lane in range(64):
                        e = step * (64 * i + lane)
                        blk, rest = e // (g.RH * M), e % (g.RH * M)
                        n = (mw + blk * R + rd * g.RH + rest // M) * M + rest % M
                        for k in range(step):
                            assert image[g.ypos(e) + k] == n + k and n + k not in seen
                            seen.add(n + k)
                # a wave's round is RH-item runs; the wave's two rounds together one run of 512 outputs
        assert seen == set(range(2048))


@pytest.mark.parametrize("M", MS)
def test_staged_transform_is_the_inverse_dft_at_bitreversed_columns(M):
    stages = M.bit_length() - 1
    rng = np.random.default_rng(M + 1)
    X = (rng.standard_normal(M) + 1j * rng.standard_normal(M)).astype(np.complex64)
    tw = twiddles(M)
    a = X.copy()
    lanes = np.arange(M)
    for s in range(stages):
        half = M >> (s + 1)
        b = a[lanes ^ half]
        sgn = np.where(lanes & half, -1.0, 1.0).astype(np.float32)
        t = (a * sgn + b).astype(np.complex64)
        a = (t * tw[s]).astype(np.complex64) if s < stages - 1 else t
    row = np.empty(M, np.complex64)
    for p in range(M):
        row[col_entry(M, bitrev(p, stages))] = a[p]
    v = np.array([row[col_entry(M, r)] for r in range(M)])
    ref = np.fft.ifft(X.astype(np.complex128)) * M
    assert np.max(np.abs(v - ref)) <= 1e-6 * np.max(np.abs(ref))
