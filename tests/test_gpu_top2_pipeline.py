"""hamming_top2_mfma_kernel's tile loop (orbx_top2.hip) against the oracle, exactly.

A wave's four query tiles form two groups; one group's MFMAs of a candidate
tile are in the pipe while the other group's top-2 update of the tile before
issues, and the candidate fragments are read from LDS one tile ahead, in two
register sets; the next chunk's candidates are expanded into the other LDS
buffer inside the tiles, and the chunk after next is loaded behind them. The
seams this adds are between the two groups, between the two fragment sets (odd
/ even tiles of a 128-candidate chunk), at the chunk barrier (the last update
of a chunk is carried across it), between chunks staged in front of the loop
and inside it, and at the drain after the last chunk; the ragged last tile is
masked after its MFMAs. The
cases put candidate counts and exact ties on every one of them, in both
candidate halves of a workgroup. Expected values are the oracle's sequential
scan: best index, best distance and second distance, equal bit for bit, for
the MFMA kernel and for the VALU one (ORBX_TOP2_VALU=1).
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -0x5A5A5A5B  # the int32 of the bytes A5 A5 A5 A5

KERNELS = ["mfma", "valu"]
NB_SHAPES = [0, 1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 511, 513]
NA_EDGES = [1, 31, 33, 255, 256, 257]


def _select(monkeypatch, kernel):
    if kernel == "valu":
        monkeypatch.setenv("ORBX_TOP2_VALU", "1")
    else:
        monkeypatch.delenv("ORBX_TOP2_VALU", raising=False)


class _Launch:
    """The device copies of one launch's pairs; run() launches into prefilled outputs."""

    def __init__(self, pkg, sets, cap_a=None):
        from orb_slam_cuda_amd import _lib
        self._lib = _lib
        self.P = len(sets)
        self.cap_a = cap_a or max(1, max(len(a) for a, _ in sets))
        self.cap_b = max(1, max(len(b) for _, b in sets))
        A_ = np.zeros((self.P, self.cap_a, 32), np.uint8)
        B_ = np.zeros((self.P, self.cap_b, 32), np.uint8)
        nA = np.array([len(a) for a, _ in sets], np.int32)
        nB = np.array([len(b) for _, b in sets], np.int32)
        for p, (a, b) in enumerate(sets):
            A_[p, :len(a)], B_[p, :len(b)] = a, b
        self.dev = [_lib.DeviceArray(x.nbytes) for x in (A_, B_, nA, nB)]
        for d, x in zip(self.dev, (A_, B_, nA, nB)):
            d.upload(x)
        self.outs = [_lib.DeviceArray(self.P * self.cap_a * 4) for _ in range(3)]
        self.m = pkg.ORBmatcher(0.9, True, max_pairs=self.P, max_kps=max(self.cap_a, self.cap_b))

    def run(self, prefill=True):
        _lib, L = self._lib, self._lib.lib()
        if prefill:
            for o in self.outs:
                o.upload(np.full(self.P * self.cap_a, FILL, np.int32))
        dA, dB, dnA, dnB = self.dev
        _lib.check(L.orbm_hamming_top2(self.m.handle, C.c_void_p(dA.ptr), self.cap_a * 32, C.c_void_p(dnA.ptr),
                                       self.cap_a, C.c_void_p(dB.ptr), self.cap_b * 32, C.c_void_p(dnB.ptr), self.P,
                                       *(C.c_void_p(o.ptr) for o in self.outs), None), matcher=True)
        L.orbx_stream_synchronize(None)
        return tuple(o.download((self.P, self.cap_a), np.int32) for o in self.outs)


def _check(O, sets, got, refs=None):
    """Every pair equals the oracle's scan; nothing written at rows >= nA[p]."""
    bi, bd, sd = got
    for p, (a, b) in enumerate(sets):
        ri, rd, rs = refs[p] if refs is not None else O.hamming_top2(a, b)
        n = len(a)
        assert np.array_equal(bd[p, :n], rd), ("best distance", p, len(a), len(b))
        assert np.array_equal(sd[p, :n], rs), ("second distance", p, len(a), len(b))
        assert np.array_equal(bi[p, :n], ri), ("best index", p, len(a), len(b))
        for x in (bi, bd, sd):
            assert (x[p, n:] == FILL).all(), ("written beyond the query count", p)


_REFS = {}


def _shape_sets(O):
    """The pipeline-shape launch and its oracle results, computed once per module run."""
    if "shape" not in _REFS:
        rng = np.random.default_rng(20)
        A = rng.integers(0, 256, (257, 32), dtype=np.uint8)
        sets = [(A, rng.integers(0, 256, (nb, 32), dtype=np.uint8)) for nb in NB_SHAPES]
        _REFS["shape"] = (sets, [O.hamming_top2(a, b) for a, b in sets])
    return _REFS["shape"]


# -------------------------------------------------------------- pipeline shape
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_pipeline_shapes(pkg, O, kernel, monkeypatch):
    """One launch of 24 pairs, 257 queries each (two query blocks, the second with
    one query), candidate counts from none to two chunks per half: an empty
    second half, halves of one to four tiles, odd and even tile counts, a
    ragged last tile in either half, a chunk boundary +-1."""
    _select(monkeypatch, kernel)
    sets, refs = _shape_sets(O)
    assert len(sets) == 24
    _check(O, sets, _Launch(pkg, sets).run(), refs)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_chunks_staged_inside_the_loop(pkg, O, kernel, monkeypatch):
    """Three to five chunks per half: from the third on a chunk's rows are loaded
    and staged inside the tile loop of the chunks before it. Counts at a chunk
    boundary of the first half, of the second half, and off both."""
    _select(monkeypatch, kernel)
    rng = np.random.default_rng(23)
    A = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    sets = [(A, rng.integers(0, 256, (nb, 32), dtype=np.uint8)) for nb in (767, 768, 769, 1023, 1025, 1201)]
    _check(O, sets, _Launch(pkg, sets).run())


# ---------------------------------------------------------------- query edges
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_query_edges(pkg, O, kernel, monkeypatch):
    """300 candidates against 1 ... 257 queries in one launch, and a_cap = nA = 300
    (the last query block partly filled) in another."""
    _select(monkeypatch, kernel)
    rng = np.random.default_rng(21)
    B = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    sets = [(rng.integers(0, 256, (na, 32), dtype=np.uint8), B) for na in NA_EDGES]
    _check(O, sets, _Launch(pkg, sets).run())
    full = [(rng.integers(0, 256, (300, 32), dtype=np.uint8), B)]
    _check(O, full, _Launch(pkg, full, cap_a=300).run())


# --------------------------------------------------------------------- ties
def _tie_pairs():
    """One pair per (query, seam): the launch's queries are the same 8 rows in every
    pair, the planted candidates differ. Returns (sets, description per pair)."""
    rng = np.random.default_rng(22)
    nb = 300
    per = (nb + 1) // 2
    A = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    sets, what = [], []

    def fresh():
        return rng.integers(0, 256, (nb, 32), dtype=np.uint8)

    # two exact copies of query i astride a tile, a fragment set, a chunk and the two halves
    for lo, hi in ((31, 32), (63, 64), (127, 128), (per - 1, per)):
        for i in range(len(A)):
            B = fresh()
            B[lo] = B[hi] = A[i]
            sets.append((A, B))
            what.append(("copies", i, lo, hi))
    # one bit flipped at the end of a tile, the exact copy at the start of the next one
    for lo, hi in ((31, 32), (63, 64), (127, 128), (per - 1, per)):
        for i in range(len(A)):
            B = fresh()
            B[lo] = A[i]
            B[lo, i] ^= np.uint8(1 << (i % 8))
            B[hi] = A[i]
            sets.append((A, B))
            what.append(("flipped", i, lo, hi))
    # complements: distance 256 beside ordinary candidates, and alone
    B = fresh()
    for i in range(len(A)):
        B[16 * i + 5] = ~A[i]
    sets.append((A, B))
    what.append(("complement", -1, 0, 0))
    for i in range(len(A)):
        sets.append((A[i:i + 1], ~A[i:i + 1]))
        what.append(("complement alone", i, 0, 0))
    return sets, what, per


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_ties_across_the_seams(pkg, O, kernel, monkeypatch):
    """Exact copies of a query at candidate indices (31, 32), (63, 64), (127, 128)
    and (per - 1, per): the lower index wins and the second distance is 0. A
    copy with one bit flipped in front of an exact copy in the next tile: the
    later, exact one wins with second distance 1. Complements: distance 256 is
    never the best beside other candidates, and alone gives no match."""
    _select(monkeypatch, kernel)
    sets, what, per = _tie_pairs()
    assert per == 150
    got = _Launch(pkg, sets).run()
    _check(O, sets, got)
    bi, bd, sd = got
    for p, (kind, i, lo, hi) in enumerate(what):
        if kind == "copies":
            assert (bi[p, i], bd[p, i], sd[p, i]) == (lo, 0, 0), (p, kind, i, lo, hi)
        elif kind == "flipped":
            assert (bi[p, i], bd[p, i], sd[p, i]) == (hi, 0, 1), (p, kind, i, lo, hi)
        elif kind == "complement":
            assert (bd[p, :8] < 256).all() and (bi[p, :8] % 16 != 5).all()
        else:
            assert (bi[p, 0], bd[p, 0], sd[p, 0]) == (-1, 256, 256), (p, kind, i)


# ----------------------------------------------------- the same launch twice
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_same_launch_twice(pkg, O, kernel, monkeypatch):
    """The pipeline-shape launch twice into prefilled outputs, the second time over
    the first's results: identical, and nothing written at rows >= nA[p]."""
    _select(monkeypatch, kernel)
    sets, refs = _shape_sets(O)
    sets = [(a[:200 + p], b) for p, (a, b) in enumerate(sets)]  # nA[p] < a_cap: rows to leave alone
    launch = _Launch(pkg, sets, cap_a=257)
    first = launch.run()
    second = launch.run(prefill=False)
    for x, y in zip(first, second):
        assert np.array_equal(x, y)
    _check(O, sets, second, [tuple(r[:200 + p] for r in ref) for p, ref in enumerate(refs)])


# ------------------------------------------------------------ diagnostics guard
@pytest.mark.parametrize("switch", ["ORBX_M_NOSTAGE", "ORBX_M_NOTOP2", "ORBX_M_NOMFMA"])
def test_timing_switches_need_diag_build(switch):
    """The timing-only builds of the MFMA kernel (no staging / no top-2 update / no
    MFMA: wrong results) compile only with -DORBX_DIAG, which stamps the library."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "orb_slam_cuda_amd", "csrc", "orbx_top2.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-fsyntax-only", "-std=c++17",
                        "-I" + os.path.join(ROOT, "include"), "-D" + switch, src],
                       capture_output=True, text=True)
    assert r.returncode != 0
    assert "result-changing diagnostic switches need -DORBX_DIAG" in r.stderr
