"""k_fir_xlat's LDS image and work mapping, checked on the host (CPU only) for every decimation:
the geometry nsh_fir_xlat_plan_create picks (restated here), the bank model of
tests/test_lds_layouts.py for the per-lane ds_read_b64 of the sample walk, and an index-level
walk of the kernel's loops: every (output, tap) pair is met exactly once with the right window
sample, no tap outside [0, L) is touched, and no LDS entry past the allocation is read."""
import pytest

from tests.test_lds_layouts import B64, cycles

KBLOCK = 256


def geometry(D, L):
    """(R, S, T, a, Lc, entries) as nsh_fir_xlat_plan_create computes them."""
    if D <= 4:
        R, S = 8, 1
    elif D <= 8:
        R, S = 4, 1
    elif D <= 16:
        R, S = 4, 2
    elif D <= 32:
        R, S = 4, 4
    else:
        R, S = 2, 4
    T = KBLOCK * R // S
    a = 0
    while (R * D) % (2 << a) == 0:
        a += 1
    Lc = ((L + S - 1) // S + 7) // 8 * 8
    wn = T * D + L + 8
    return R, S, T, a, Lc, wn + (wn >> a) + 1


@pytest.mark.parametrize("D", range(1, 65))
def test_window_reads_conflict_free_and_fit(D):
    for L in (1, 127, 1024):
        R, S, T, a, Lc, entries = geometry(D, L)
        assert T * D <= 8192 and entries * 8 <= 160 * 1024
        if a >= 3 and L <= 800:
            assert 2 * entries * 8 <= 160 * 1024        # two workgroups per CU
        stride = R * D + (R * D >> a)
        assert stride % 2 == 1
        for j in (0, 5, 8, (R - 1) * D + L - 1):
            for wave in range(4 // S):                  # the waves of one part
                addr = [8 * ((wave * 64 + lane) * stride + j + (j >> a)) for lane in range(64)]
                assert cycles(addr, B64, 8) == 2, (D, L, j)


@pytest.mark.parametrize("D,L", [(1, 1), (1, 127), (2, 127), (3, 8), (5, 33), (7, 1024), (8, 127), (10, 200),
                                 (16, 9), (16, 127), (33, 40), (64, 2), (64, 1024)])
def test_walk_meets_every_tap_once(D, L):
    R, S, T, a, Lc, entries = geometry(D, L)
    count = (T - 1) * D + L                              # staged samples: window positions [0, count)
    groups = KBLOCK // S
    for grp in (0, 1, groups // 2, groups - 1):
        met = {}
        for part in range(S):
            qlo, qhi = part * Lc, min(L, part * Lc + Lc)
            if qlo >= qhi:
                continue
            pbase = grp * (R * D + (R * D >> a))
            for jb in range(qlo, (R - 1) * D + qhi, 8):
                assert jb % 8 == 0
                for i in range(8):
                    j = jb + i
                    assert pbase + j + (j >> a) < entries
                    s = grp * R * D + j                  # the window position that entry holds
                    assert pbase + j + (j >> a) == s + (s >> a)
                    for r in range(R):
                        q = j - r * D
                        if qlo <= q < qhi:               # both the 8-tap path and the edge path
                            assert s < count
                            key = (grp * R + r, L - 1 - q)
                            assert key not in met
                            met[key] = s
        assert len(met) == R * L
        for (o, k), s in met.items():
            assert s == o * D + (L - 1) - k              # x[(m0 + o) D - k] at window position 0 = m0 D - (L-1)
    assert (S - 1) * T <= entries                        # the partial sums reuse the window
