"""nsh_psd_cf (k_psd<N, LIN>, k_psd_sum) where tests/test_gpu_psd.py cannot see it fail: that file
never averages more than 2 P + 3 = 67 frames (nseg <= 3, so k_psd_sum's strided loop takes one trip
and the host's 16-group form never runs), its bound g = (K + 2) 2^-24 is wider than one lost frame
from K of a few hundred on, with K > 1 its rows never leave one workgroup at the sizes that hold
several frames a team, NSH_PSD_SEGMENT is never set, and no frame overflows fp32.

Below, P is nsh_psd_segment, F, TEAMS and TILE are geom<N>'s (F = max(1024 / N, 1) frames of a team,
TILE = plan.tile rows of a workgroup) and nseg = ceil(K / 32).

Exact frames. x_f[n] = a_f delta[n] + b_f / N + c_f (-1)^n / N with a_f, b_f, c_f complex integers
whose parts lie in [-5, 5]: every sample is exact in fp32 and X_f[k] = a_f + b_f [k = 0] +
c_f [k = N / 2], so three classes of bins carry different small integers, |X_f[k]|^2 <= 200 is an
integer, and with K max |X|^2 < 2^24 and a power-of-two scale every partial sum of every order of
additions is exact: the output is float32(scale * integer sum), compared in bits. A lost, repeated
or misplaced frame changes an integer. The precondition -- nsh_fft_c2c returns exactly those X_f
on these very frames -- is asserted first (Exact.check_transform); it holds for the mixed frames at
every size used here, so the pure-frame form (each frame only a, only b or only c; Exact(pure=True))
is not needed by any test and PURE_SIZES is empty.

The chain model (chain_model) restates, in numpy fp32, the order of additions written down in
nsh_psd.hip and DESIGN.md section 4.9; test 1 checks the model itself without a GPU and test 4 holds
the kernel to it bit for bit on noise.

run() of tests/test_gpu_psd.py is used throughout: it checks the guard floats around the output and
ends the input exactly at the end of its allocation."""
import numpy as np
import pytest

from newsched_amd import nsh
from tests.gpu_util import bits, hann
from tests.psd_ref import balanced_segment, fft_of, frames_per_team, reference, run, segment, signal

gpu = pytest.mark.gpu
KSEG = 32     # kSegment of nsh_psd.hip: the most frames of a segment by default
RANGE = 5     # parts of a_f, b_f, c_f lie in [-RANGE, RANGE]: |X_f[k]|^2 <= 8 RANGE^2 = 200
PURE_SIZES = frozenset()  # sizes at which the mixed frames' transform is not exact (none)


# ---------------------------------------------------------------- exact frames

class Exact:
    """nframes exact frames of N samples (module docstring) and their integer powers per bin class."""

    def __init__(self, N, nframes, seed=11, pure=None):
        pure = N in PURE_SIZES if pure is None else pure
        rng = np.random.default_rng(100 * seed + N)
        co = rng.integers(-RANGE, RANGE + 1, (3, 2, nframes)).astype(np.float64)
        if pure:
            keep = np.arange(nframes) % 3
            for i in range(3):
                co[i][:, keep != i] = 0
        a, b, c = (co[i][0] + 1j * co[i][1] for i in range(3))
        x = np.empty((nframes, N), np.complex64)
        x[:, 0::2] = ((b + c) / N)[:, None]
        x[:, 1::2] = ((b - c) / N)[:, None]
        x[:, 0] += a.astype(np.complex64)
        self.N, self.nframes, self.pure = N, nframes, pure
        self.x = x.reshape(-1)
        self.x.setflags(write=False)
        self.X = np.stack([a, a + b, a + c]).astype(np.complex64)  # other bins, bin 0, bin N / 2
        Xd = np.stack([a, a + b, a + c])
        self.pw = Xd.real * Xd.real + Xd.imag * Xd.imag             # float64 integers, (3, nframes)
        assert np.all(self.pw == np.rint(self.pw)) and self.pw.max() <= 8 * RANGE * RANGE
        self.checked = False

    def check_transform(self, torch):
        """The precondition: nsh_fft_c2c gives exactly X_f on these frames."""
        if self.checked:
            return
        N = self.N
        Y = fft_of(torch, self.x, N).reshape(-1, N)
        ok = np.all(Y[:, 0] == self.X[1]) and np.all(Y[:, N // 2] == self.X[2])
        Y[:, 0] = Y[:, N // 2] = self.X[0]
        ok = ok and np.all(Y == self.X[0][:, None])
        assert ok, "precondition: the transform of the exact frames is not exact at N = %d (pure = %s)" % (N, self.pure)
        self.checked = True

    def take(self, K, nvec):
        assert nvec * K <= self.nframes
        return self.x[:nvec * K * self.N]

    def want(self, K, nvec, scale, shift):
        """float32(scale * integer sum) per bin, (nvec, N)."""
        N = self.N
        assert K * self.pw.max() < 2 ** 24 and np.log2(scale) == np.rint(np.log2(scale)), "not exact in fp32"
        s = self.pw[:, :nvec * K].reshape(3, nvec, K).sum(axis=2)
        w = np.repeat(s[0][:, None], N, axis=1)
        w[:, 0], w[:, N // 2] = s[1], s[2]
        w = (scale * w).astype(np.float32)
        return np.fft.fftshift(w, axes=1) if shift else w


def walk_nvec(N, tile):
    """Vectors of a call whose rows (nvec nseg of them) reach a third row group and whose count is no
    multiple of F, so that teams straddle vectors and the last team is part empty."""
    F = frames_per_team(N)
    nvec = 2 * tile + 3
    return nvec + 1 if F > 1 and nvec % F == 0 else nvec


def tile_of(N):
    p = nsh.PsdPlan(N, 1)
    t = p.tile
    p.close()
    assert t == max(256 // max(N // 16, 64), 1) * frames_per_team(N)  # TEAMS F of geom<N>
    return t


# ---------------------------------------------------------------- the chain of additions, in numpy

def sum_geometry(N, nseg):
    """(G, bins) of k_psd_sum as nsh_psd_plan_create derives lgb: up to 16 groups of lanes share a
    vector's rows, a group covers at least 16 bins."""
    groups = 1
    while groups < 16 and groups < nseg:
        groups *= 2
    bins = min(256 // groups, N)
    return 256 // bins, bins


def chain_model(q, N, P, scale):
    """The documented order in fp32. q: per-frame powers (nvec, K, B) float32, not negative (B bins
    that all take the route of a bin of an N-point plan). Frames are added in order within a segment
    of P, starting from 0; one segment: times scale. More: group g of G adds segments g, g + G, .. in
    order starting from 0, the group sums are added in group order starting from group 0's, times
    scale. Missing frames of a short last segment and missing segments of a group are zeros: x + 0 = x
    in bits for x >= 0, which is also what the kernels do."""
    q = np.asarray(q)
    assert q.dtype == np.float32
    nvec, K, B = q.shape
    nseg = -(-K // P)
    if nseg * P != K:
        z = np.zeros((nvec, nseg * P, B), np.float32)
        z[:, :K] = q
        q = z
    q = q.reshape(nvec, nseg, P, B)
    seg = np.zeros((nvec, nseg, B), np.float32)
    for s in range(P):
        seg = seg + q[:, :, s]
    scale = np.float32(scale)
    if nseg == 1:
        out = seg[:, 0] * scale
    else:
        G, _ = sum_geometry(N, nseg)
        trips = -(-nseg // G)
        if trips * G != nseg:
            z = np.zeros((nvec, trips * G, B), np.float32)
            z[:, :nseg] = seg
            seg = z
        seg = seg.reshape(nvec, trips, G, B)
        gs = np.zeros((nvec, G, B), np.float32)
        for t in range(trips):
            gs = gs + seg[:, t]
        tot = gs[:, 0]
        for g in range(1, G):
            tot = tot + gs[:, g]
        out = tot * scale
    assert out.dtype == np.float32
    return out


LONG_KS = [225, 257, 481, 513, 1025, 4097, 65535, 65536]  # nseg 8, 9, 16, 17, 33, 129, 2048, 2048


# ---- 1. the model itself ----------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 64, 1024])
def test_chain_model_on_the_cpu(N):
    """No GPU. One-hot powers: frame f alone has power 2^(f mod 20), in a bin of its own, so that bin
    of the model's output is 2^(f mod 20) exactly when the frame enters the sum once and only once --
    every frame for K up to 4097, and at K = 65535 and 65536 (where a bin per frame would take 16 GiB)
    the frames around both ends, around every boundary of the first and the last segments and of the
    second trip of a group, and 160 random ones; there a bin of all ones must also come out as K, the
    count of additions with multiplicity. On random integer powers in [0, 200] the model equals the
    integer sum bit for bit. Sizes 16, 64 and 1024 take every (G, bins) pair the plan derives."""
    rng = np.random.default_rng(3 + N)
    seen = set()
    for K in [1, 7, 32, 33, 67] + LONG_KS:
        P = balanced_segment(K, KSEG)
        nseg = -(-K // P)
        G, bins = sum_geometry(N, nseg)
        assert G * bins == 256 and bins <= N and (G == 16 or nseg <= 8)
        seen.add((nseg, G))
        if K <= 4097:
            sel = np.arange(K)
        else:
            edges = np.array([0, P, 2 * P, G * P, 2 * G * P, (nseg - G) * P, (nseg - 1) * P, K])
            near = (edges[:, None] + np.arange(-3, 3)[None, :]).ravel()
            sel = np.unique(np.concatenate([near[(near >= 0) & (near < K)], rng.integers(0, K, 160)]))
        q = np.zeros((1, K, sel.size + 1), np.float32)
        q[0, sel, np.arange(sel.size)] = 2.0 ** (sel % 20)
        q[0, :, sel.size] = 1.0
        out = chain_model(q, N, P, 0.5)[0]
        assert np.array_equal(out[:-1], (0.5 * 2.0 ** (sel % 20)).astype(np.float32)), (N, K)
        assert out[-1] == 0.5 * K, (N, K)
        q = rng.integers(0, 201, (2, K, 24)).astype(np.float32)
        want = (0.25 * q.astype(np.float64).sum(axis=1)).astype(np.float32)
        assert K * 200 < 2 ** 24
        assert np.array_equal(bits(chain_model(q, N, P, 0.25), np.float32), bits(want, np.float32)), (N, K)
    assert {n for n, _ in seen} >= {1, 2, 3, 8, 9, 16, 17, 33, 129, 2048}
    if N == 16:
        assert all(g == 16 for n, g in seen if n > 1)  # 16 bins a group whatever nseg is


@pytest.mark.parametrize("pure", [False, True])
def test_exact_frames_on_the_cpu(pure):
    """No GPU. The helper against numpy's float64 FFT: the frames transform to the three integer
    classes, want() is the plain sum of |X|^2 over each vector, and the chain model gives the same
    bits on those powers -- for the mixed frames and for the pure ones held in reserve."""
    for N in (16, 64, 2048):
        ex = Exact(N, 4 * 67, pure=pure)
        X = np.fft.fft(ex.x.astype(np.complex128).reshape(-1, N), axis=1)
        assert np.max(np.abs(X - np.rint(X.real) - 1j * np.rint(X.imag))) < 1e-9
        X = np.rint(X.real) + 1j * np.rint(X.imag)
        assert np.all(X[:, 0] == ex.X[1]) and np.all(X[:, N // 2] == ex.X[2]) and np.all(X[:, 1] == ex.X[0])
        assert len({tuple(r) for r in ex.pw.T}) > 20 and np.all(ex.pw.max(axis=1) > 0)
        p = X.real * X.real + X.imag * X.imag
        for K, nvec in ((67, 4), (7, 5)):
            for shift in (False, True):
                plain = (0.25 * p[:nvec * K].reshape(nvec, K, N).sum(axis=1)).astype(np.float32)
                model = chain_model(p[:nvec * K].astype(np.float32).reshape(nvec, K, N), N, balanced_segment(K, KSEG), 0.25)
                if shift:
                    plain, model = np.fft.fftshift(plain, axes=1), np.fft.fftshift(model, axes=1)
                want = ex.want(K, nvec, 0.25, shift)
                assert np.array_equal(bits(want, np.float32), bits(plain, np.float32)), (N, K, shift)
                assert np.array_equal(bits(want, np.float32), bits(model, np.float32)), (N, K, shift)


# ---- 2. the row walk ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N", [16, 32, 64, 128, 256, 512, 2048])
def test_row_walk_exact(torch_cuda, N):
    """Exact frames, K in {1, 3, F + 1, P + 1, 2 P + 3}, 2 TILE + 3 vectors (one more where that is
    a multiple of F), so the rows of a call fill more than two row groups, teams other than the first
    straddle vectors and short last segments fall into later groups; under the default grid cap (one
    group a workgroup) and under caps 1 and 2 (a workgroup walks on to later groups with K > 1), with
    and without shift: every output equals the integer sum bit for bit."""
    torch = torch_cuda
    P, F = segment(N), frames_per_team(N)
    ks = sorted({min(k, 65536) for k in (1, 3, F + 1, P + 1, 2 * P + 3)})
    nvec = walk_nvec(N, tile_of(N))
    ex = Exact(N, nvec * max(ks))
    ex.check_transform(torch)
    scale = 0.25
    for K in ks:
        x = ex.take(K, nvec)
        for shift in (False, True):
            plan = nsh.PsdPlan(N, K, None, shift, scale)
            assert plan.segment == balanced_segment(K, P)
            assert nvec * -(-K // plan.segment) >= 2 * plan.tile + 3
            want = bits(ex.want(K, nvec, scale, shift), np.float32)
            for cap in (0, 1, 2):
                plan.grid_cap(cap)
                out = bits(run(torch, plan, x), np.float32)
                bad = np.argwhere(out != want)
                assert bad.size == 0, (plan.kernel, K, shift, cap, "first wrong (vector, bin):", bad[0], len(bad))
            plan.close()


# ---- 3. long averages ---------------------------------------------------------------------------
LONG = [(N, K) for N in (16, 64) for K in LONG_KS] + [(1024, 257), (1024, 513), (1024, 1025), (8192, 513)]


@gpu
@pytest.mark.parametrize("N,K", LONG)
def test_long_averages_exact(torch_cuda, N, K, monkeypatch):
    """nseg = 8, 9, 16, 17, 33, 129 and 2048: k_psd_sum below and above 16 groups of lanes, a second
    and later trips of its strided loop (nseg > G), a short last segment 2047 segments from the first
    (K = 65535) and the largest K. Exact frames, 2 vectors (1 from K = 65535 on), with and without
    shift: integer sums bit for bit. The K = 513 and 1025 shapes run again on 3 vectors with scratch
    for one vector's rows, so every batch is one vector."""
    torch = torch_cuda
    nvec = 1 if K >= 65535 else 2
    batched = K in (513, 1025)
    ex = Exact(N, (3 if batched else nvec) * K)
    ex.check_transform(torch)
    scale = 2.0 ** -3
    for shift in (False, True):
        plan = nsh.PsdPlan(N, K, None, shift, scale)
        assert plan.segment == balanced_segment(K, KSEG)
        out = run(torch, plan, ex.take(K, nvec))
        assert np.array_equal(bits(out, np.float32), bits(ex.want(K, nvec, scale, shift), np.float32)), (plan.kernel, K, shift)
        plan.close()
    if batched:
        nseg = -(-K // balanced_segment(K, KSEG))
        monkeypatch.setenv("NSH_PSD_SCRATCH_BYTES", str(nseg * N * 4))
        small = nsh.PsdPlan(N, K, None, True, scale)
        monkeypatch.delenv("NSH_PSD_SCRATCH_BYTES")
        out = run(torch, small, ex.take(K, 3))
        assert np.array_equal(bits(out, np.float32), bits(ex.want(K, 3, scale, True), np.float32)), \
            (small.kernel, K, "batches of one vector")
        small.close()


# ---- 4. the order of the additions --------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N", [16, 128, 512, 1024, 4096])
def test_chain_of_additions_is_the_documented_one(torch_cuda, N):
    """This test pins internals on purpose: it must be updated together with any change of the
    summation order (k_psd's accumulation, k_psd_sum, the derivation of lgb in nsh_psd_plan_create,
    kSegment), and with the text of nsh_psd.hip and DESIGN.md section 4.9 that states the order.

    Noise and two tones under a Hann window. The per-frame powers q_f[k] come from a K = 1, scale 1,
    unshifted plan of the same size and window: this kernel's own 0 + (re^2 + im^2). chain_model adds
    them in fp32 in the documented order; the (N, K) plan's output must equal it in bits, for 3
    vectors, K in {7, 33, 67, 257, 513, 1025} (1025 left out at N = 4096), with and without shift."""
    torch = torch_cuda
    w = hann(N)
    ks = [k for k in (7, 33, 67, 257, 513, 1025) if not (N == 4096 and k == 1025)]
    x = signal(N, 3 * max(ks), 9)
    one = nsh.PsdPlan(N, 1, w, False, 1.0)
    q = run(torch, one, x)
    one.close()
    assert np.all(q >= 0) and np.all(np.isfinite(q))
    for K in ks:
        for shift in (False, True):
            plan = nsh.PsdPlan(N, K, w, shift)
            assert plan.segment == balanced_segment(K, KSEG)
            model = chain_model(q[:3 * K].reshape(3, K, N), N, plan.segment, np.float32(plan.scale))
            if shift:
                model = np.fft.fftshift(model, axes=1)
            out = run(torch, plan, x[:3 * K * N])
            differ = int(np.sum(bits(out, np.float32) != bits(model, np.float32)))
            assert differ == 0, (plan.kernel, K, shift, "bins that differ from the documented chain:", differ)
            plan.close()


# ---- 5. noise across row groups -----------------------------------------------------------------
WALK = [(N, K) for N in (16, 64, 256, 512) for K in (5, KSEG + 1)]


@gpu
@pytest.mark.parametrize("N,K", WALK)
def test_noise_within_the_bound_across_groups(torch_cuda, N, K):
    """The float64 reference and the bound B of tests/test_gpu_psd.py on noise and tones under a Hann
    window, K = 5 and P + 1, over 2 TILE + 3 vectors (more than two row groups), with and without
    shift: err / B <= 1 in every bin; the worst ratio is printed (DESIGN.md section 4.9 records it).
    Data that is not flat across bins, so a wrong bin order in a later group shows."""
    torch = torch_cuda
    assert K in (5, segment(N) + 1)
    w = hann(N)
    nvec = walk_nvec(N, tile_of(N))
    x = signal(N, nvec * K, 10)
    for shift in (False, True):
        plan = nsh.PsdPlan(N, K, w, shift)
        assert nvec * -(-K // plan.segment) >= 2 * plan.tile + 3
        out = run(torch, plan, x).astype(np.float64)
        ref, B = reference(x, N, K, w, 1.0 / K, shift)
        ratio = np.max(np.abs(out - ref) / B)
        print("5/groups N=%d K=%d shift=%d %s nvec=%d: worst err/B %.3g" % (N, K, shift, plan.kernel, nvec, ratio))
        assert ratio <= 1.0, (plan.kernel, K, shift, ratio)
        plan.close()


# ---- 6. cut invariance across row groups --------------------------------------------------------
@gpu
@pytest.mark.parametrize("N,K", WALK + [(64, 513)])
def test_cut_invariance_across_groups(torch_cuda, N, K):
    """A call of 2 TILE + 3 vectors: vector 0, vector TILE - 1, vector TILE and the last one are each
    bit-identical to the same vector in a call of its own, and the whole call is bit-identical to
    itself with the input 1 sample and the output 3 floats further on."""
    torch = torch_cuda
    w = hann(N)
    plan = nsh.PsdPlan(N, K, w, True)
    nvec = walk_nvec(N, plan.tile)
    x = signal(N, nvec * K, 10)
    V = K * N
    whole = run(torch, plan, x)
    for j in (0, plan.tile - 1, plan.tile, nvec - 1):
        own = run(torch, plan, x[j * V:(j + 1) * V])
        assert np.array_equal(bits(own[0], np.float32), bits(whole[j], np.float32)), (plan.kernel, K, j)
    assert np.array_equal(bits(whole, np.float32), bits(run(torch, plan, x, in_off=1, out_off=3), np.float32)), (plan.kernel, K)
    plan.close()


# ---- 7. NSH_PSD_SEGMENT -------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N,K,nvec", [(16, 4096, 66), (64, 1000, 18), (1024, 300, 6)])
def test_segment_override(torch_cuda, N, K, nvec, monkeypatch):
    """NSH_PSD_SEGMENT = 0 (one segment of all K frames), 1 (nseg = K), 5 and 64 at plan creation:
    nsh_psd_segment is K, respectively balanced_segment(K, s), and the sums of exact frames are the
    integer sums bit for bit. At 0 and N = 16 a team's 64 rows lie 63 * 4096 frames apart, about
    33 MB: the largest per-lane offset this suite reaches. The kernel's limit of 2^29 bytes between a
    team's rows takes a 512 MB input and stays out of scope here."""
    torch = torch_cuda
    ex = Exact(N, nvec * K)
    ex.check_transform(torch)
    x = ex.take(K, nvec)
    scale = 0.5
    want = bits(ex.want(K, nvec, scale, False), np.float32)
    for s in (0, 1, 5, 64):
        monkeypatch.setenv("NSH_PSD_SEGMENT", str(s))
        plan = nsh.PsdPlan(N, K, None, False, scale)
        monkeypatch.delenv("NSH_PSD_SEGMENT")
        assert plan.segment == (K if s == 0 else balanced_segment(K, s)), (plan.kernel, s)
        assert np.array_equal(bits(run(torch, plan, x), np.float32), want), (plan.kernel, s)
        plan.close()


# ---- 8. overflow ----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N", [64, 1024, 4096])
def test_overflowing_power_stays_in_its_vector(torch_cuda, N):
    """Finite samples only. (a) One frame in the middle of vector 1 of 3 carries 2^65 at sample N / 2
    (where the Hann window is 1): |X[k]| = 2^65 in every bin, |X|^2 = inf. (b) The first and the last
    frame of vector 1 carry 1.25 2^63 (1 + i) there: each frame's power is 1.5625 2^127, finite
    (asserted on a K = 1 plan), two of them overflow -- in k_psd for K = 5, only in k_psd_sum for
    K = P + 3, where they lie in different segments. Either way vector 1 is +inf in every bin, also
    in dB, and vectors 0 and 2 are bit-identical to the clean run."""
    torch = torch_cuda
    P = segment(N)
    w = hann(N)
    assert w[N // 2] == 1.0
    for K in (5, P + 3):
        x = signal(N, 3 * (P + 3), 6)[:3 * K * N]
        V = K * N
        one_big = np.array(x)
        one_big[V + (K // 2) * N + N // 2] = 2.0 ** 65
        two_half = np.array(x)
        two_half[V + N // 2] = two_half[V + (K - 1) * N + N // 2] = 1.25 * 2.0 ** 63 * (1 + 1j)
        assert np.all(np.isfinite(one_big.view(np.float32))) and np.all(np.isfinite(two_half.view(np.float32)))
        each = nsh.PsdPlan(N, 1, w, False, 1.0)
        q = run(torch, each, two_half[V:2 * V])
        each.close()
        assert np.all(np.isfinite(q)) and np.all(q[[0, K - 1]] > 2.0 ** 127) and np.all(q[1:K - 1] < 2.0 ** 40)
        for db in (False, True):
            plan = nsh.PsdPlan(N, K, w, False, None, db)
            clean = run(torch, plan, x)
            assert np.all(np.isfinite(clean))
            for name, z in (("one frame", one_big), ("the sum", two_half)):
                out = run(torch, plan, z)
                assert np.all(np.isposinf(out[1])), (plan.kernel, K, db, name)
                assert np.array_equal(bits(out[[0, 2]], np.float32), bits(clean[[0, 2]], np.float32)), (plan.kernel, K, db, name)
            plan.close()
