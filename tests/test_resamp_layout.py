"""k_resamp<R,P>'s LDS image and work mapping, checked on the host (CPU only) for every instantiation
and for I, D over {1, 2, 3, 5, 7, 16, 31, 48, 63, 64}: the geometry of nsh_resamp.hip (restated here:
the instantiation, the tile, the padding the plan chooses), the bank model of
tests/test_lds_layouts.py for the per-lane ds_read_b64 of the samples, and an index-level walk of the
kernel's loops: every (output, tap) pair is met exactly once with the right stream sample and the
right tap, no tap at or past L is touched, no LDS entry past the allocation is read or written, every
output of a tile is stored exactly once."""
import functools

import numpy as np
import pytest

KBLOCK, MAX_TILE_IN = 256, 8192
VALUES = [1, 2, 3, 5, 7, 16, 31, 48, 63, 64]
PAIRS = [(i, d) for i in VALUES for d in VALUES]

# The worst number of different entries that the 32 lanes of one ds_read_b64 group put on one bank
# pair. k_resamp<8,1> (D <= I, packed image, a lane's units G apart): the samples of consecutive lanes
# never decrease and rise by at most one, so 32 lanes span at most 32 consecutive entries:
# conflict-free. The others (a lane's units consecutive, padding s + (s >> a) picked by the plan): the
# lanes read floor(r D / I) apart inside a group of units and R D apart between groups, two strides
# at once, and one shift cannot make both odd: 1 wherever I = 1 (one stride), else at most WORST_ANY.
WORST_ANY = 3


def tile(I, D):
    """(R, G) of nsh_resamp_plan_create: the instantiation and the groups of R units per workgroup"""
    R = 8 if D <= 2 * I else 4 if D <= 4 * I else 2 if D <= 8 * I else 1
    return R, max(1, min(KBLOCK // I, MAX_TILE_IN // (R * D)))


def linear(I, D):
    """k_resamp<8,1>: the packed image, a lane's units G apart"""
    return D <= I


def worst_multiplicity(I, D, a):
    """worst_multiplicity() of nsh_resamp.hip: over the 32-lane groups and the window offsets c < 64"""
    R, G = tile(I, D)
    w = np.arange(G * I)
    s = (w // I) * (1 if linear(I, D) else R) * D + (w % I) * D // I   # k_resamp<8,1>: lanes of one r are D apart
    worst = 1
    for c in range(64):
        e = c + s + ((c + s) >> a)
        for l0 in range(0, G * I, 32):
            u = np.unique(e[l0:l0 + 32])                # equal entries are a broadcast
            worst = max(worst, int(np.bincount(u % 32).max()))
    return worst


@functools.lru_cache(maxsize=None)
def padding(I, D):
    """(a, worst multiplicity): the a in {31 (no padding), 6, ..., 1} with the smallest worst case, the
    larger a on a tie; k_resamp<8,1> has no padding"""
    if linear(I, D):
        return 31, worst_multiplicity(I, D, 31)
    best = None
    for a in (31, 6, 5, 4, 3, 2, 1):
        m = worst_multiplicity(I, D, a)
        if best is None or m < best[1]:
            best = (a, m)
    return best


class Geom:
    """the plan of nsh_resamp_plan_create"""

    def __init__(self, I, D, L, a=None):
        self.I, self.D, self.L = I, D, L
        self.Q = -(-L // I)
        self.R, self.G = tile(I, D)
        self.U = self.G * self.R
        self.a = padding(I, D)[0] if a is None else a
        wn = self.U * D + self.Q - 1
        self.hs_at = (max(wn + (wn >> self.a) + 1, self.U * I) + 1) // 2 * 2
        self.lds_bytes = self.hs_at * 8 + self.Q * I * 4

    def entry(self, s):
        return s + (s >> self.a)

    def lane(self, w):
        """(g, r, base, phi) of lane w < G I"""
        g, r = divmod(w, self.I)
        base, phi = divmod(r * self.D, self.I)
        return g, r, base, phi

    def unit(self, g, t):
        """the t-th unit of the lanes of group g"""
        return g + t * self.G if linear(self.I, self.D) else g * self.R + t


def test_instantiations_and_tiles():
    seen = set()
    for I, D in PAIRS + [(i, d) for i in range(1, 65) for d in (1, 2, 4, 8, 9, 16, 17, 33, 64)]:
        g = Geom(I, D, 1024, a=1)                       # a = 1: the largest image the plan can choose
        seen.add(g.R)
        assert 1 <= g.G * I <= KBLOCK                   # one output-in-unit index per lane, no second pass
        assert g.U * D <= max(MAX_TILE_IN, g.R * D) and g.U * I <= 2048
        assert g.lds_bytes <= 116 * 1024                # within the CU's 160 KiB, whatever L
        assert g.hs_at % 2 == 0 and g.hs_at >= g.U * I  # the taps 16-byte aligned, past the output image
    assert seen == {1, 2, 4, 8}
    # (64, 1) and (1, 64) stay within a few workgroups per CU
    assert (160 * 1024) // Geom(64, 1, 1024).lds_bytes >= 4
    assert (160 * 1024) // Geom(1, 64, 1024).lds_bytes >= 2


@pytest.mark.parametrize("I,D", PAIRS)
def test_sample_reads_bank_multiplicity(I, D):
    g = Geom(I, D, 127)
    a, worst = padding(I, D)
    print(f"  I={I} D={D}: k_resamp<{g.R},{int(linear(I, D))}> G={g.G} a={a} worst multiplicity {worst}")
    assert worst <= WORST_ANY
    if linear(I, D):
        assert g.R == 8 and a == 31 and worst == 1
    elif I == 1:
        assert worst == 1


def test_unpadded_image_would_conflict():
    """why the image is padded: the lanes of a decimator by 4 are R D = 16 samples apart, 16 to a bank
    pair; with a = 4, k_fir_xlat's choice (16 is the largest power of two in R D), the stride is 17"""
    assert tile(1, 4) == (4, 256)
    assert worst_multiplicity(1, 4, 31) == 16
    assert padding(1, 4) == (4, 1)
    assert padding(1, 31) == (31, 1)                    # an odd stride needs no padding
    # k_resamp<8,1>'s mapping past D = I: two or three entries to a bank pair (measured slower)
    for I, D in ((2, 3), (4, 5), (1, 2)):
        w = np.arange(tile(I, D)[1] * I)
        s = (w // I) * D + (w % I) * D // I
        assert max(int(np.bincount(np.unique(s[l:l + 32]) % 32).max()) for l in range(0, w.size, 32)) in (2, 3)


@pytest.mark.parametrize("I,D", PAIRS)
@pytest.mark.parametrize("L", [1, 2, 63, 64, 1000, 1024])
def test_walk_meets_every_tap_once(I, D, L):
    g = Geom(I, D, L)
    Q, H, R = g.Q, g.Q - 1, g.R
    count = g.U * D + H                                 # staged samples: window position i at entry(i)
    assert g.entry(count - 1) < g.hs_at
    qall = L // I
    stored = {}
    lanes = range(g.G * I) if g.G * I <= 24 else sorted({0, 1, I - 1, I, g.G * I // 2, g.G * I - 1})
    for w in lanes:
        grp, r, base, phi = g.lane(w)
        s0 = H + g.unit(grp, 0) * D + base
        met = {}
        for q in list(range(qall)) + ([qall] if qall < Q and phi + qall * I < L else []):
            k = phi + q * I
            assert k < L and k < Q * I                  # the right tap, inside hs[]
            for t in range(R):
                s = s0 + (g.unit(grp, t) - g.unit(grp, 0)) * D - q
                assert 0 <= s < count and g.entry(s) < g.hs_at
                assert (t, k) not in met
                met[(t, k)] = s
        for t in range(R):
            n = g.unit(grp, t) * I + r                  # the output's place in the tile
            taps = [k for k in range(L) if (n * D - k) % I == 0]
            assert sorted(k for (tt, k) in met if tt == t) == taps
            for k in taps:                              # u[nD - k] = x[(nD - k) / I]; window position 0 is x[-H]
                assert met[(t, k)] == (n * D - k) // I + H
            assert n < g.U * I <= g.hs_at and n not in stored
            stored[n] = w
    if len(lanes) == g.G * I:
        assert sorted(stored) == list(range(g.U * I))   # every output of the tile, once


@pytest.mark.parametrize("I,D", PAIRS)
def test_every_output_stored_once(I, D):
    g = Geom(I, D, 127)
    tile_out = g.U * I
    image = set()
    for w in range(g.G * I):
        grp, r, _, _ = g.lane(w)
        for t in range(g.R):
            e = g.unit(grp, t) * I + r
            assert e not in image and e < g.hs_at
            image.add(e)
    assert image == set(range(tile_out))
    for vec in ((True, False) if tile_out % 2 == 0 else (False,)):
        for n_out in (tile_out, tile_out - 1, 1):       # a full tile, and the stream's last one
            seen = []
            step = 2 if vec else 1
            for tid in range(KBLOCK):
                for e in range(step * tid, tile_out, step * KBLOCK):
                    if e + step - 1 < n_out:
                        seen += list(range(e, e + step))
                    elif e < n_out:
                        seen.append(e)
            assert sorted(seen) == list(range(n_out))
