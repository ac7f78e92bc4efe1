"""The segment-table arithmetic of csrc/pp_segments.h, on the CPU (the header is plain C++; the kernels compile the same text).

Every context describes its complexes by one table ``off[0 .. n_seg]`` (first rows, then the total).  Here the header's functions
against (a) a brute-force linear scan on well-formed tables, uniform (a padded [B][L] batch) and ragged (a packed one), (b) on
tables that break the contract, a NumPy restatement of what the kernels computed before the header existed, when each carried its
own copy: the packed segment fill, the seeded-noise row table, the proximal / loss row ranges -- a malformed table must keep giving
the clamped answers it gave, (c) the padded forms ``n / L``, ``s * L`` those kernels had next to the packed ones, and (d) the
decoy-group functions against a restatement of the header comment of csrc/pp_ensemble.hip, whose kernels and those of
csrc/pp_recombine.hip each carried a copy of them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("segments") / "libsegments_check.so")
    subprocess.run(["g++", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    os.path.join(ROOT, "tests", "native", "segments_check.cpp")], check=True)
    return ctypes.CDLL(so)


class Table:
    def __init__(self, h, off):
        self.h, self.off = h, np.ascontiguousarray(off, dtype=np.int32)
        self.p, self.n_seg = self.off.ctypes.data_as(ctypes.c_void_p), len(off) - 1

    def of_row(self, n):
        return self.h.seg_of_row(self.p, self.n_seg, int(n))

    def start(self, s, n):
        return self.h.seg_start(self.p, int(s), int(n))

    def rows(self, s, N):
        out = np.zeros(2, np.int32)
        self.h.seg_rows(self.p, int(s), int(N), out.ctypes.data_as(ctypes.c_void_p))
        return int(out[0]), int(out[1])

    def group(self, g, D, N):
        """(consistent?, first consensus row, length, first row of decoy 0) of group g."""
        out = np.zeros(4, np.int32)
        self.h.group_rows(self.p, int(g), int(D), int(N), out.ctypes.data_as(ctypes.c_void_p))
        return bool(out[0]), int(out[1]), int(out[2]), int(out[3])

    def group_of(self, G, D, N, crow):
        return self.h.group_of_cons_row(self.p, int(G), int(D), int(N), int(crow))

    def decoy_row0(self, g, D, N, d):
        return self.h.decoy_row0(self.p, int(g), int(D), int(N), int(d))

    def fill(self, N, max_len):
        out = np.zeros((N, 2), np.int32)
        self.h.seg_fill_all(self.p, self.n_seg, int(N), int(max_len), out.ctypes.data_as(ctypes.c_void_p))
        return out


# ---- brute force, for tables that keep the contract (0 = off[0] <= off[1] <= ... <= off[n_seg] = N) ----------------------------------
def scan_of_row(off, n):
    """The last s in 0 .. n_seg - 1 with off[s] <= n, by looking at every entry."""
    hits = [s for s in range(len(off) - 1) if off[s] <= n]
    return hits[-1] if hits else 0


def check_well_formed(t, off, max_len):
    N = int(off[-1])
    for s in range(t.n_seg):
        assert t.rows(s, N) == (off[s], off[s + 1]), (off, s)
    fill = t.fill(N, max_len)
    for n in range(N):
        s = scan_of_row(off, n)
        assert off[s] <= n < off[s + 1]
        assert t.of_row(n) == s, (off, n)
        assert t.start(s, n) == off[s]
        assert tuple(fill[n]) == (off[s], off[s + 1] - off[s]), (off, n)


def test_uniform_tables_are_the_padded_forms(harness):
    """A padded [B][L] context: table s * L.  The seg fill gives ((n / L) * L, L), the noise table (n / L, n % L), the loss and the
    proximal kernels rows s * L .. (s + 1) * L -- what the padded branches computed without a table."""
    for B in range(1, 6):
        for L in range(1, 71):
            off = [s * L for s in range(B + 1)]
            t, N = Table(harness, off), B * L
            check_well_formed(t, off, L)
            n = np.arange(N)
            assert np.array_equal(t.fill(N, L), np.stack([(n // L) * L, np.full(N, L)], 1))
            for r in range(N):
                s = t.of_row(r)
                assert (s, r - t.start(s, r)) == (r // L, r % L)
            for s in range(B):
                assert t.rows(s, N) == (s * L, (s + 1) * L)


def test_ragged_tables_against_a_linear_scan(harness):
    rng = np.random.default_rng(15)
    for _ in range(200):
        lens = rng.integers(1, 201, int(rng.integers(1, 9)))
        off = [0] + [int(v) for v in np.cumsum(lens)]
        check_well_formed(Table(harness, off), off, int(lens.max()))


# ---- tables that break the contract: the arithmetic each kernel carried before it was shared, restated --------------------------------
def old_search(off, n_seg, n):
    lo, hi = 0, n_seg - 1
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if off[mid] <= n:
            lo = mid
        else:
            hi = mid - 1
    return lo


def old_fill_seg_packed(off, n_seg, N, max_len, n):
    lo = old_search(off, n_seg, n)
    start, ln = off[lo], off[lo + 1] - off[lo]
    start = 0 if start < 0 else (n if start > n else start)
    ln = max_len if ln > max_len else ln
    if start + ln > N:
        ln = N - start
    if n >= start + ln:
        ln = n - start + 1 if n - start + 1 <= max_len else max_len
    return start, ln


def old_rng_row(off, n_seg, n):
    lo = old_search(off, n_seg, n)
    start = off[lo]
    start = 0 if start < 0 else (n if start > n else start)
    return lo, n - start


def old_seg_rows(off, s, N):
    a, b = off[s], off[s + 1]
    a = 0 if a < 0 else (N if a > N else a)
    b = a if b < a else (N if b > N else b)
    return a, b


def malformed_tables():
    yield "decreasing", [0, 40, 25, 60, 90], 90, 40
    yield "decreasing from the start", [50, 30, 10, 0], 50, 30
    yield "negative", [-5, 10, 30, 64], 64, 40
    yield "all negative", [-30, -20, -10, -1], 20, 12
    yield "above N", [0, 20, 500, 700], 64, 30
    yield "first entry above N", [100, 120, 140], 64, 20
    yield "last entry short of N", [0, 20, 33, 50], 64, 20
    yield "last entry beyond N", [0, 20, 33, 80], 64, 47
    yield "zero-length segment", [0, 20, 20, 45, 64], 64, 25
    yield "zero-length first and last", [0, 0, 30, 64, 64], 64, 34
    yield "longer than max_len", [0, 50, 64], 64, 20
    yield "first row not 0", [7, 30, 64], 64, 34
    rng = np.random.default_rng(151)
    for k in range(300):
        n_seg, N = int(rng.integers(1, 9)), int(rng.integers(1, 300))
        yield f"random {k}", [int(v) for v in rng.integers(-40, N + 60, n_seg + 1)], N, int(rng.integers(1, N + 1))


def test_malformed_tables_keep_their_clamped_answers(harness):
    for name, off, N, max_len in malformed_tables():
        t = Table(harness, off)
        fill = t.fill(N, max_len)
        for n in range(N):
            s = t.of_row(n)
            assert s == old_search(off, t.n_seg, n), (name, n)
            assert (s, n - t.start(s, n)) == old_rng_row(off, t.n_seg, n), (name, n)
            start, ln = (int(v) for v in fill[n])
            assert (start, ln) == old_fill_seg_packed(off, t.n_seg, N, max_len, n), (name, n)
            # what the clamps are for: the segment is inside the batch and the launch's max_len, and reaches its row if max_len lets it
            assert 0 <= start <= n and 1 <= ln <= max_len and start + ln <= N and (n < start + ln or ln == max_len), (name, n)
        for s in range(t.n_seg):
            a, b = t.rows(s, N)
            assert (a, b) == old_seg_rows(off, s, N), (name, s)
            assert 0 <= a <= b <= N


# ---- decoy groups: G * D segments read as G groups of D decoys (pp_group_rows, pp_group_of_cons_row, pp_decoy_row0) --------------------
# Restated from the header comment of csrc/pp_ensemble.hip (LAYOUT and A TABLE THAT BREAKS THE CONTRACT), by looking at every
# segment: segment g * D + d is decoy d of group g; rows are the clamped ones; the consensus row of (g, r) is (first row of decoy 0)
# / D + r; a group is consistent when its D clamped segments have one length >= 1 and its consensus rows lie inside the N / D.
def brute_group(off, g, D, N):
    segs = [old_seg_rows(off, g * D + d, N) for d in range(D)]
    lens = [b - a for a, b in segs]
    row0 = segs[0][0]
    base = row0 // D
    consensus_rows = range(base, base + lens[0])
    ok = len(set(lens)) == 1 and lens[0] >= 1 and all(0 <= r < N // D for r in (consensus_rows[0], consensus_rows[-1]))
    return ok, base, lens[0], row0


def brute_group_of(off, G, D, N, crow):
    """The last g whose first consensus row is <= crow, as the kernels have always searched for it: by bisection, which on a table
    whose first rows do not ascend is not the last such g of a linear scan -- and must stay what it was."""
    lo, hi = 0, G - 1
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if old_seg_rows(off, mid * D, N)[0] // D <= crow:
            lo = mid
        else:
            hi = mid - 1
    return lo


def group_tables():
    """(name, off, N, D, what every group must come out as: consistent or not, or None = only the comparison)"""
    yield "G = 2, D = 3, lengths 5 and 1", [0, 5, 10, 15, 16, 17, 18], 18, 3, [True, True]
    yield "D = 1", [0, 7, 20, 21], 21, 1, [True, True, True]
    yield "one decoy shorter", [0, 4, 7, 11, 12, 13, 14, 16, 18, 20], 20, 3, [False, True, True]
    yield "one decoy longer, in the last group", [0, 2, 4, 6, 8, 10, 13], 13, 2, [True, True, False]
    yield "consensus rows past N / D", [0, 3, 6, 14, 12, 20], 20, 2, [True, False]
    yield "negative and beyond N", [-5, 4, 8, 30, 40], 16, 2, [True, False]
    yield "zero-length group", [0, 0, 0, 6, 12], 12, 2, [False, True]
    for name, off, N, _ in malformed_tables():
        for D in range(1, len(off)):
            if (len(off) - 1) % D == 0:
                yield f"{name}, D = {D}", off, N, D, None


def test_decoy_groups_against_the_ensemble_header(harness):
    for name, off, N, D, want in group_tables():
        t = Table(harness, off)
        G = t.n_seg // D
        got = [t.group(g, D, N) for g in range(G)]
        for g in range(G):
            ok, base, ln, row0 = brute_group(off, g, D, N)
            assert got[g] == (ok, base, ln, row0), (name, g)
            for d in range(D):
                assert t.decoy_row0(g, D, N, d) == old_seg_rows(off, g * D + d, N)[0], (name, g, d)
            if ok:           # what the rule is for: every row of every decoy is a row of the batch, every consensus row one of the N / D
                assert 0 <= base and base + ln <= N // D
                assert all(0 <= t.decoy_row0(g, D, N, d) and t.decoy_row0(g, D, N, d) + ln <= N for d in range(D))
        if want is not None:
            assert [g[0] for g in got] == want, name
        for crow in range(-2, N // D + 3):
            assert t.group_of(G, D, N, crow) == brute_group_of(off, G, D, N, crow), (name, crow)


def test_consensus_rows_of_well_formed_ensembles_find_their_group(harness):
    """Groups of D equal decoys back to back: consensus rows 0 .. N / D - 1, each in the group a linear scan of the lengths gives."""
    rng = np.random.default_rng(16)
    for _ in range(100):
        D, lens = int(rng.integers(1, 6)), rng.integers(1, 80, int(rng.integers(1, 7)))
        off = [0] + [int(v) for v in np.cumsum(np.repeat(lens, D))]
        t, N, G = Table(harness, off), off[-1], len(lens)
        first = np.concatenate([[0], np.cumsum(lens)])
        for g in range(G):
            assert t.group(g, D, N) == (True, int(first[g]), int(lens[g]), int(first[g]) * D)
            assert [t.decoy_row0(g, D, N, d) for d in range(D)] == [int(first[g]) * D + d * int(lens[g]) for d in range(D)]
        for crow in range(N // D):
            assert t.group_of(G, D, N, crow) == int(np.searchsorted(first, crow, side="right")) - 1
