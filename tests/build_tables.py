"""Tables for the device plan builder (csrc/wagg_build.hip) at the edges of its sort, scans and runs, and the fp64
restatement they are checked against.  Not a conftest, no fixtures: tests/test_build_tables_host.py checks everything here
without a GPU, tests/test_gpu_build_small.py and tests/fuzz_gpu.py (build_case) hand the tables to DensePlan.from_segments /
DensePlan.from_csr.

A table is (cell, code, w) in TABLE ORDER plus what its constructor promises (`meta`).  The three routes of one table:
  coo         the rows as they are                                  -> general sort
  csr         rows stably sorted by cell (columns as they come)     -> general sort (unless the columns happen to ascend)
  csr_sorted  rows stably sorted by (cell, code)                    -> one-pass partition when nothing is dropped
A stable sort keeps the rows of one (cell, region) pair in table order, so all three give the same pair sums bit for bit.

The restatement (`reference`): rows with code < 0 or a NaN weight leave; the weights of a repeated pair add in table order
(np.add.at over the flat pair index: unbuffered, element after element -- pinned against a Python loop by the host test);
nnz = distinct surviving pairs; den[r] = math.fsum of region r's pair sums, with the bound n_r 2^-53 sum |pair sum| for any
fixed fp64 summation order (n_r - 1 roundings, each at most 2^-53 of a partial sum that never exceeds sum |pair sum|).

Order-sensitive runs.  With A = 2^60 (one ulp = 256) and distinct small integers s0 .. s3 in [1, 31] -- any four of them add
to less than 128 = half an ulp of A, so A absorbs them -- the rows of a repeated pair carry
  length 3   A -A s0              table-order sum s0
  length 4   A s0 -A s1           s1
  length 5   s0 A s1 -A s2        s2
  length 6   s0 s1 A s2 -A s3     s3
A swap of the first two rows of a run can never show in a sum (a + b = b + a), and some others cannot either.  Shares of the
neighbour transpositions (i, i + 1), 0-based, whose sequential fp64 sum differs from the table order's (measured by
`transposition_shares`, asserted by the host test):
  length 3: 1 of 2 (i = 1)      length 4: 2 of 3 (i = 1, 2)      length 5: 2 of 4 (i = 2, 3)      length 6: 2 of 5 (i = 3, 4)
so every i >= 1 is shown by at least one pattern: i = 1 by lengths 3 and 4, i = 2 by 4 and 5, i = 3 by 5 and 6, i = 4 by 6.
Random runs take the lengths 3, 4, 5, 6 in turn: every pattern goes to a quarter of the runs (asserted: at least a fifth,
on tables with 100 runs or more).  Longer runs (7 rows and more) must not forget their early rows, so they are L mod 5 small integers followed by blocks
  A b -A c e      b in [129, 191], c and e in [65, 95]
whose effect stays in the sum as a multiple of 256: b, alone between A and -A, rounds to 256; c and e, added to each other
exactly outside the brackets (130 .. 190), round to 256 together at the next A, but each alone rounds to 0, and b + c + e
(259 .. 381) rounds to 256, not 512.  Every block but the last adds 512, the sum of the run is 512 (q - 1) + 256 + c_q + e_q, and
of the five neighbour swaps of a block (the one with the next block's A included) all but c <-> e change the sum by 256 for
good -- 4 of 5, anywhere in a run of 20,000 rows (asserted by the host test).  No tie occurs: no rounded fraction is 128."""
import math

import numpy as np

A_BIG = 2.0 ** 60
SMALL_MAX = 31
BG_SCALE = 65536.0                                               # single rows: uniform(0.1, 1) * BG_SCALE
PATTERNS = {3: ("A", "-A", 0), 4: ("A", 0, "-A", 1), 5: (0, "A", 1, "-A", 2), 6: (0, 1, "A", 2, "-A", 3)}
PROBE_TOL = {np.float32: 2.0 ** -22, np.float64: 2.0 ** -51}     # fl(W), fl(den), one division (tests/test_gpu_dense_forms_small.py)
ROUND, WAVE_SLICE, SORT_TILE, SCAN_TILE, BLOCK = 64, 1024, 8192, 2048, 256
KEY_DROPPED = 2 ** 64 - 1


# ---- the builder's geometry, restated (csrc/wagg_spmm.hip: spmm_geometry; csrc/wagg_build.h: EntryKeyGeom) ----------------------
def geometry(G, R):
    """(n_rb, rw, n_chunks): region blocks of 16 waves x at most 43 regions, balanced; chunks of 128 cells"""
    n_rb = -(-R // 688)
    return n_rb, -(-R // (16 * n_rb)), -(-G // 128)


def key_range(G, R):
    n_rb, rw, n_chunks = geometry(G, R)
    return n_rb * n_chunks * 16 * 128 * rw


def passes_for(rng_):
    """8-bit digits covering [0, range]"""
    bits = int(rng_).bit_length()
    return 1 if bits == 0 else (bits + 7) // 8


def key_of(cell, region, G, R):
    n_rb, rw, n_chunks = geometry(G, R)
    cell, region = np.asarray(cell, dtype=np.int64), np.asarray(region, dtype=np.int64)
    wv, j = region // rw, region % rw
    bucket = ((wv >> 4) * n_chunks + (cell >> 7)) * 16 + (wv & 15)
    return (bucket * 128 + (cell & 127)) * rw + j


def decode(k, G, R):
    n_rb, rw, n_chunks = geometry(G, R)
    k = np.asarray(k, dtype=np.int64)
    j, k = k % rw, k // rw
    cic, k = k & 127, k >> 7
    wave, k = k & 15, k >> 4
    chunk, rb = k % n_chunks, k // n_chunks
    return chunk * 128 + cic, (rb * 16 + wave) * rw + j


def chunk_bin(cell, region, G, R):
    """bin of the one-pass partition inside the pair's chunk: region block x 16 + wave"""
    n_rb, rw, n_chunks = geometry(G, R)
    return np.asarray(region, dtype=np.int64) // rw


# ---- order-sensitive weights ----------------------------------------------------------------------------------------------------
def seq_sum(ws):
    s = 0.0
    for x in ws:
        s += float(x)
    return s


def pattern_rows(L, smalls):
    """(k, L) weights of k runs of length L in 3 .. 6 from (k, 4) small integers"""
    out = np.empty((len(smalls), L))
    for p, s in enumerate(PATTERNS[L]):
        out[:, p] = A_BIG if s == "A" else -A_BIG if s == "-A" else smalls[:, s]
    return out


def draw_smalls(rng, k):
    """(k, 4) distinct integers in [1, SMALL_MAX] per row"""
    return np.argsort(rng.random((k, SMALL_MAX)), axis=1)[:, :4] + 1.0


def run_weights(L, rng):
    """the weights of one run of any length, in table order"""
    if L == 1:
        return rng.uniform(0.1, 1.0, 1) * BG_SCALE
    if L == 2:
        return draw_smalls(rng, 1)[0, :2]
    if L <= 6:
        return pattern_rows(L, draw_smalls(rng, 1))[0]
    q, rem = divmod(L, 5)
    blocks = np.stack([np.full(q, A_BIG), rng.integers(129, 192, q).astype(np.float64), np.full(q, -A_BIG),
                       rng.integers(65, 96, q).astype(np.float64), rng.integers(65, 96, q).astype(np.float64)], axis=1)
    return np.concatenate([draw_smalls(rng, 1)[0, :rem], blocks.ravel()])


def differs(a, b):
    """beyond the fp64 probe's tolerance (an exact 0 where the table-order sum is 0)"""
    return abs(a - b) > PROBE_TOL[np.float64] * abs(b)


def detectable_swaps(ws):
    """the i (0-based) at which swapping rows i and i + 1 changes the sequential fp64 sum beyond the tolerance"""
    ws = [float(x) for x in ws]
    base, out = seq_sum(ws), []
    for i in range(len(ws) - 1):
        sw = ws[:i] + [ws[i + 1], ws[i]] + ws[i + 2:]
        if differs(seq_sum(sw), base):
            out.append(i)
    return out


def transposition_shares(n_draws=50, seed=0):
    """{L: (set of i detectable in EVERY draw, number of transpositions)} for the patterns in use"""
    rng = np.random.default_rng(seed)
    out = {}
    for L in PATTERNS:
        always = set(range(L - 1))
        for _ in range(n_draws):
            always &= set(detectable_swaps(run_weights(L, rng)))
        out[L] = (always, L - 1)
    return out


# ---- tables ---------------------------------------------------------------------------------------------------------------------
class Table:
    def __init__(self, name, G, R, cell, code, w, **meta):
        self.name, self.G, self.R = name, int(G), int(R)
        self.cell = np.ascontiguousarray(cell, dtype=np.int32)
        self.code = np.ascontiguousarray(code, dtype=np.int32)
        self.w = np.ascontiguousarray(w, dtype=np.float64)
        assert self.cell.shape == self.code.shape == self.w.shape and self.cell.ndim == 1
        for a in (self.cell, self.code, self.w):
            a.setflags(write=False)
        self.meta = meta
        self._ref = None

    n = property(lambda self: len(self.cell))
    keep = property(lambda self: (self.code >= 0) & ~np.isnan(self.w))
    n_valid = property(lambda self: int(self.keep.sum()))

    def coo(self):
        return self.cell, self.code, self.w

    def csr(self, sort_columns=False, order=None):
        """(rowptr, col, val): rows stably sorted by cell, or by (cell, code)"""
        if order is None:
            order = np.lexsort((self.code, self.cell)) if sort_columns else np.argsort(self.cell, kind="stable")
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(self.cell, minlength=self.G))]).astype(np.int64)
        return rowptr, self.code[order], self.w[order]

    def ref(self):
        if self._ref is None:
            self._ref = reference(self.cell, self.code, self.w, self.G, self.R)
        return self._ref

    def sorted_keys(self):
        """the keys of the valid rows in the builder's sorted order"""
        k = self.keep
        return np.sort(key_of(self.cell[k], self.code[k], self.G, self.R), kind="stable")

    def expect_one_pass(self, rowptr, col, general_sort=False):
        """build_sorted_entries' rule: CSR, at most 1024 bins, nothing dropped, ascending columns, no over-long chunk"""
        n_rb, rw, n_chunks = geometry(self.G, self.R)
        if general_sort or n_rb * 16 > 1024 or self.n_valid != self.n or self.n == 0:
            return 0
        inner = np.ones(self.n, dtype=bool)
        inner[rowptr[:-1][rowptr[:-1] < self.n]] = False                 # first entry of every row
        if (np.diff(col.astype(np.int64), prepend=0)[inner] < 0).any():
            return 0
        longest = max(int(rowptr[min(128 * (c + 1), self.G)] - rowptr[128 * c]) for c in range(n_chunks))
        return int(longest <= max(64 * SORT_TILE, 8 * (self.n // n_chunks + 1)))


class Ref:
    pass


def reference(cell, code, w, G, R):
    """The fp64 restatement: see the module's docstring."""
    cell, code, w = np.asarray(cell, dtype=np.int64), np.asarray(code, dtype=np.int64), np.asarray(w, dtype=np.float64)
    keep = (code >= 0) & ~np.isnan(w)
    flat = cell[keep] * R + code[keep]
    r = Ref()
    r.G, r.R = G, R
    r.flat, inv = np.unique(flat, return_inverse=True)
    r.ws = np.zeros(len(r.flat))
    np.add.at(r.ws, inv.ravel(), w[keep])                        # element after element: table order
    r.nnz = len(r.flat)
    r.pair_cell, r.pair_region = r.flat // R, r.flat % R
    order = np.argsort(r.pair_region, kind="stable")
    bounds = np.searchsorted(r.pair_region[order], np.arange(R + 1))
    r.n_r = np.diff(bounds)
    r.den = np.array([math.fsum(r.ws[order[bounds[i]:bounds[i + 1]]]) for i in range(R)])
    r.den_tol = r.n_r * 2.0 ** -53 * np.bincount(r.pair_region, weights=np.abs(r.ws), minlength=R)
    return r


def reference_loop(cell, code, w, R):
    """{(cell, region): sum in table order} by a plain Python loop"""
    out = {}
    for c, k, x in zip(cell.tolist(), code.tolist(), w.tolist()):
        if k >= 0 and x == x:
            out[(c, k)] = out.get((c, k), 0.0) + x
    return out


def amplitudes(cells):
    """a = +-2^k, k cycling through -3 .. 3, the sign alternating"""
    g = np.asarray(cells, dtype=np.int64)
    return np.where(g % 2 == 0, 1.0, -1.0) * 2.0 ** (g % 7 - 3)


def probe_cells(t):
    """every cell for G <= 4096; else the cells that hold a pair (at most 512, cell 0 and G - 1 among them) and 32 that hold none"""
    if t.G <= 4096:
        return np.arange(t.G)
    used = np.unique(np.concatenate([t.cell[t.keep], [0, t.G - 1]]))
    assert len(used) <= 512
    free = np.setdiff1d(np.linspace(1, t.G - 2, 200).astype(np.int64), used)[:32]
    assert len(free) == 32
    return np.sort(np.concatenate([used, free]))


def probe_matrices(ref, cells):
    """(W, has) of the probed cells: (len(cells), R)"""
    cells = np.asarray(cells)
    W = np.zeros((len(cells), ref.R))
    has = np.zeros((len(cells), ref.R), dtype=bool)
    row = np.searchsorted(cells, ref.pair_cell)
    row[row == len(cells)] = 0
    hit = cells[row] == ref.pair_cell
    W[row[hit], ref.pair_region[hit]] = ref.ws[hit]
    has[row[hit], ref.pair_region[hit]] = True
    return W, has


class Readback:
    """what a test reads from a plan: nnz, den (fp64, [R]) and the probe's result for `cells` ([len(cells), R])"""
    def __init__(self, nnz, den, probe):
        self.nnz, self.den, self.probe = int(nnz), np.asarray(den, dtype=np.float64), np.asarray(probe)


def ideal_readback(ref, cells, dtype=np.float64):
    """the readback of a builder that computes exactly what `ref` states"""
    W, _ = probe_matrices(ref, cells)
    with np.errstate(divide="ignore", invalid="ignore"):
        probe = (amplitudes(cells)[:, None] * W.astype(dtype).astype(np.float64) / ref.den.astype(dtype).astype(np.float64)[None, :])
    return Readback(ref.nnz, ref.den, probe.astype(dtype))


def check_counts(ref, rb):
    """nnz exact; den within the fsum bound"""
    assert rb.nnz == ref.nnz, "nnz %d, expected %d" % (rb.nnz, ref.nnz)
    assert rb.den.shape == ref.den.shape
    bad = ~(np.abs(rb.den - ref.den) <= ref.den_tol)
    assert not bad.any(), "den of region %d: got %r, fsum %r, bound %r" % (
        np.flatnonzero(bad)[0], rb.den[bad][0], ref.den[bad][0], ref.den_tol[bad][0])


def check_readback(ref, cells, rb, dtype=np.float64):
    """THE comparison of the GPU tests: check_counts, then check_probe."""
    check_counts(ref, rb)
    check_probe(ref, cells, rb, dtype)


def check_probe(ref, cells, rb, dtype=np.float64):
    """Every probed weight within PROBE_TOL of the table-order pair sum (divided by the plan's own fp64 den, as
    tests/test_gpu_dense_forms_small.py does), an exact 0 where the sum is 0 or no pair exists, the IEEE result where
    den == 0."""
    W, has = probe_matrices(ref, cells)
    got = np.asarray(rb.probe, dtype=np.float64)
    assert got.shape == W.shape
    a = amplitudes(cells)
    den = rb.den
    with np.errstate(divide="ignore", invalid="ignore"):
        exp = a[:, None] * W / den[None, :]
    ok = rb.den != 0
    okc = np.broadcast_to(ok[None, :], W.shape)
    zero = okc & (W == 0)                                        # no pair, or a table-order sum of exactly 0
    wrong = zero & (got != 0.0)
    assert not wrong.any(), "%d results that must be 0 are not, first at (probe row, region) %s (cell %d): %r" % (
        wrong.sum(), np.argwhere(wrong)[0], cells[np.argwhere(wrong)[0][0]], got[tuple(np.argwhere(wrong)[0])])
    with np.errstate(invalid="ignore"):
        err = np.abs(got - exp)
        bad = okc & (W != 0) & ~(err <= PROBE_TOL[dtype] * np.abs(exp))
    assert not bad.any(), "%d of %d weights wrong, first at (probe row, region) %s (cell %d): got %r, expected %r" % (
        bad.sum(), has.sum(), np.argwhere(bad)[0], cells[np.argwhere(bad)[0][0]], got[tuple(np.argwhere(bad)[0])],
        exp[tuple(np.argwhere(bad)[0])])
    np.testing.assert_array_equal(np.isnan(got[:, ~ok]), np.isnan(exp[:, ~ok]))
    inf = np.isinf(exp[:, ~ok])
    np.testing.assert_array_equal(got[:, ~ok][inf], exp[:, ~ok][inf])


# ---- the general constructor: runs of given lengths on distinct pairs, scattered or in CSR order ----------------------------------
def draw_lengths(rng, n_rows, p_run):
    """run lengths adding to n_rows: 1 with probability 1 - p_run, else 3, 4, 5, 6 in turn (the last one is what is left)"""
    if n_rows == 0:
        return np.zeros(0, dtype=np.int64)
    is_run = rng.random(n_rows) < p_run
    L = np.where(is_run, 3 + (np.cumsum(is_run) + int(rng.integers(0, 4))) % 4, 1)
    cs = np.cumsum(L)
    k = int(np.searchsorted(cs, n_rows))
    L = L[:k + 1].copy()
    L[k] = n_rows - (cs[k - 1] if k else 0)
    return L


def weights_of(lengths, rng, single=None):
    """the rows' weights run after run; `single`: weights of the one-row pairs (default uniform(0.1, 1) BG_SCALE)"""
    lengths = np.asarray(lengths, dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(lengths)])
    w = np.empty(start[-1])
    for L in np.unique(lengths):
        ids = np.flatnonzero(lengths == L)
        if L == 1:
            vals = (rng.uniform(0.1, 1.0, len(ids)) * BG_SCALE if single is None else single(rng, len(ids)))[:, None]
        elif L == 2:
            vals = draw_smalls(rng, len(ids))[:, :2]
        elif L <= 6:
            vals = pattern_rows(int(L), draw_smalls(rng, len(ids)))
        else:
            vals = np.stack([run_weights(int(L), rng) for _ in ids])
        w[(start[ids][:, None] + np.arange(L)[None, :]).ravel()] = vals.ravel()
    return w


def draw_pairs(rng, n_pairs, cells, R, empty_regions=(), must=()):
    """n_pairs distinct (cell, region), the cells from `cells`, no region of `empty_regions`, `must` among them; random order"""
    cells = np.asarray(cells, dtype=np.int64)
    regions = np.setdiff1d(np.arange(R), np.asarray(empty_regions, dtype=np.int64))
    must = list(dict.fromkeys(must))[:n_pairs]
    total = len(cells) * len(regions)
    assert n_pairs <= total, "table asks for %d distinct pairs of %d" % (n_pairs, total)
    pick = rng.choice(total, n_pairs, replace=False)
    c, r = cells[pick // len(regions)], regions[pick % len(regions)]
    if must:
        mc, mr = np.array([m[0] for m in must]), np.array([m[1] for m in must])
        other = np.flatnonzero(~np.isin(c * R + r, mc * R + mr))[:n_pairs - len(must)]
        c, r = np.concatenate([c[other], mc]), np.concatenate([r[other], mr])
        o = rng.permutation(n_pairs)
        c, r = c[o], r[o]
    assert len(np.unique(c * R + r)) == n_pairs
    return c, r


def spread_runs(pos, run_of_row, lengths):
    """{unit: ids of the runs (2 rows and more) whose rows lie in two or more units of that many input rows}"""
    start = np.concatenate([[0], np.cumsum(lengths)])[:-1]
    out = {}
    for unit in (ROUND, WAVE_SLICE, SORT_TILE):
        u = pos // unit
        lo, hi = np.minimum.reduceat(u, start), np.maximum.reduceat(u, start)
        out[unit] = np.flatnonzero((hi > lo) & (np.asarray(lengths) >= 2))
    return out


def assemble(name, G, R, pc, pr, lengths, rng, n_drop=0, order="scattered", cells=None, single=None, w=None, **meta):
    """Rows of run i on pair (pc[i], pr[i]); n_drop dropped rows (null label / NaN weight in turn, half of them on pairs that
    exist) among them.  order = "scattered": a random order that keeps every run's rows in their order; "csr": by cell, the
    columns of a cell in random order (runs in their order); "csr_sorted": by (cell, region)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n_valid = int(lengths.sum())
    if w is None:
        w = weights_of(lengths, rng, single)
    cell, code = np.repeat(pc, lengths), np.repeat(pr, lengths)
    rid = np.repeat(np.arange(len(lengths)), lengths)
    if n_drop:
        pool = np.arange(G) if cells is None else np.asarray(cells)
        dc, dr = rng.choice(pool, n_drop), rng.integers(0, R, n_drop)
        if len(pc):
            on = rng.integers(0, len(pc), n_drop // 2)
            dc[:len(on)], dr[:len(on)] = pc[on], pr[on]
        dw = rng.uniform(0.1, 1.0, n_drop) * BG_SCALE
        null = np.arange(n_drop) % 2 == 0
        dr[null & (np.arange(n_drop) % 4 == 0)] = -1 - rng.integers(0, 5)
        dr[null] = np.minimum(dr[null], -1)
        dw[~null] = np.nan
        cell, code, w = np.concatenate([cell, dc]), np.concatenate([code, dr]), np.concatenate([w, dw])
        rid = np.concatenate([rid, len(lengths) + np.arange(n_drop)])
    n = len(cell)
    pos = rng.permutation(n)
    pos = pos[np.lexsort((pos, rid))]                            # ascending inside every run: row k goes to place pos[k]
    if order != "scattered":
        # rank the rows by (cell, [region,] place): runs keep their order
        o = np.lexsort((pos, code, cell)) if order == "csr_sorted" else np.lexsort((pos, cell))
        pos = np.empty(n, dtype=np.int64)
        pos[o] = np.arange(n)
    out = [np.empty(n, dtype=a.dtype) for a in (cell, code, w)]
    for dst, src in zip(out, (cell, code, w)):
        dst[pos] = src
    t = Table(name, G, R, *out, lengths=lengths, pair_cell=np.asarray(pc), pair_region=np.asarray(pr), n_drop=n_drop, **meta)
    assert t.n_valid == n_valid and t.n == n_valid + n_drop
    t.meta["spread"] = spread_runs(pos[:n_valid], rid[:n_valid], lengths) if n_valid else {u: np.zeros(0, int) for u in (64, 1024, 8192)}
    t.meta["row_place"] = pos[:n_valid]
    # the spread that is reported is the spread the table has: look the rows of those runs up in the finished arrays
    for unit, ids in t.meta["spread"].items():
        for i in ids[:20]:
            rows = np.flatnonzero((t.cell == pc[i]) & (t.code == pr[i]) & ~np.isnan(t.w))
            assert len(rows) == lengths[i] and rows[0] // unit != rows[-1] // unit
            st = int(np.concatenate([[0], np.cumsum(lengths)])[i])
            np.testing.assert_array_equal(t.w[rows], w[st:st + lengths[i]])
    return t


def pattern_shares(t):
    """{L: share of the runs of 3 .. 6 rows that have length L}"""
    L = t.meta["lengths"]
    runs = L[(L >= 3) & (L <= 6)]
    return {k: float((runs == k).mean()) if len(runs) else 0.0 for k in PATTERNS}


def random_table(name, n_valid, n_drop, G, R, seed, p_run=0.5, order="scattered", cells=None, empty_region=None, must=None):
    """n_valid rows drawn with repetition (runs of 3 .. 6 rows on a share p_run of the pairs) + n_drop dropped rows; one
    region without a pair; the pairs with the smallest and the largest key present when there is room."""
    rng = np.random.default_rng(seed)
    pool = np.arange(G) if cells is None else np.asarray(cells)
    if empty_region is None:
        empty_region = R // 2 if R > 2 else None
    lengths = draw_lengths(rng, n_valid, p_run)
    if must is None:
        must = [(int(pool[0]), 0), (int(pool[-1]), R - 1)]
    pc, pr = draw_pairs(rng, len(lengths), pool, R, () if empty_region is None else (empty_region,), must)
    return assemble(name, G, R, pc, pr, lengths, rng, n_drop, order, cells=pool, empty_region=empty_region, must=must)


# ---- case 1: row counts at the edges of rounds, wave slices, sort tiles and scan tiles -------------------------------------------
EDGE_N = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192, 8193, 16383, 16385)


def edge_table(n, kind):
    """G = 300, R = 37.  kind "total": n rows of which a few are dropped; "valid": n valid rows and 41 dropped on top;
    "clean": n rows, none dropped (the one-pass route)."""
    drop = {"total": 0 if n < 8 else 2 + n // 50, "valid": 41, "clean": 0}[kind]
    n_valid = n - drop if kind == "total" else n
    return random_table("edge-%s-%d" % (kind, n), n_valid, drop, 300, 37, 100 * n + len(kind))


# ---- cases 2, 3: the histogram scan across its tile; scan_top_kernel's second trip -------------------------------------------------
def hist_table(n):
    return random_table("hist-%d" % n, n - 300, 300, 2048, 100, n, p_run=0.2)


def top_table(n_valid, n_drop):
    """G = 2048, R = 1100: p_run = 0.1224 gives 30 % repeated rows"""
    return random_table("top-%d+%d" % (n_valid, n_drop), n_valid, n_drop, 2048, 1100, n_valid % 1000 + n_drop, p_run=0.1224)


# ---- cases 4, 5: pass counts ------------------------------------------------------------------------------------------------------
KEY_PASS_SHAPES = ((128, 496, 2), (128, 512, 3), (32640, 512, 3), (32768, 512, 4))
REGION_PASS_SHAPES = ((300, 255, 1), (300, 256, 2), (300, 257, 2), (128, 65535, 2), (128, 65536, 3), (128, 65537, 3))


def pass_table(G, R, n_drop=200):
    """3000 valid rows in at most 400 cells (cell 0 and G - 1 among them), the smallest and the largest key present, region 0
    and R - 1 holding pairs, dropped rows"""
    rng = np.random.default_rng(G + R)
    cells = np.unique(np.concatenate([[0, G - 1], rng.choice(G, min(G, 400), replace=False)])) if G > 400 else np.arange(G)
    t = random_table("pass-%dx%d-%d" % (G, R, n_drop), 3000, n_drop, G, R, G * 7 + R, cells=cells)
    k = t.sorted_keys()
    assert k[0] == 0 and k[-1] == key_of(G - 1, R - 1, G, R) and (t.code == 0).any() and (t.code == R - 1).any()
    return t


# ---- case 6: runs for heads_kernel / coalesce_kernel ------------------------------------------------------------------------------
RUN_LENGTHS = (1, 2, 3, 4, 255, 256, 257, 8192, 8193, 20000)


def runs_table(n_drop, order="scattered", seed=6):
    """G = 256, R = 40.  In sorted order: a run that begins at the last thread of a 256-thread block (and straddles the edge),
    runs that begin at the first thread of a block, the lengths of RUN_LENGTHS, background runs of 3 .. 6 rows, and a last
    run that ends exactly at n_valid; n_drop dropped rows behind."""
    G, R = 256, 40
    rng = np.random.default_rng(seed)
    seq, marks, pos = [], {}, 0

    def put(L, mark=None):
        nonlocal pos
        if mark:
            marks[mark] = len(seq)
        seq.append(L)
        pos += L

    def pad_to(phase):
        while pos % BLOCK != phase:
            put(int(rng.integers(3, 7)) if (phase - pos) % BLOCK > 8 and rng.random() < 0.3 else 1)

    pad_to(255); put(3, "at_last_thread")
    pad_to(0); put(4, "at_first_thread")
    put(2); put(1)
    pad_to(255); put(255)
    pad_to(0); put(256, "fills_a_block")
    put(257)
    pad_to(255); put(8192, "long_at_last_thread")
    pad_to(0); put(8193)
    pad_to(130); put(20000)
    pad_to(250); put(5, "last")
    lengths = np.array(seq)
    # pairs in key order take the runs in this order
    pc, pr = draw_pairs(rng, len(lengths), np.arange(G), R, (R // 2,), [(0, 0), (G - 1, R - 1)])
    o = np.argsort(key_of(pc, pr, G, R))
    t = assemble("runs-%s-%d" % (order, n_drop), G, R, pc[o], pr[o], lengths, rng, n_drop, order, marks=marks, empty_region=R // 2)
    # the placements, from the restated key of the finished table
    k = t.sorted_keys()
    head = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    length = np.diff(np.concatenate([head, [len(k)]]))
    np.testing.assert_array_equal(length, lengths)
    for m, phase in (("at_last_thread", 255), ("at_first_thread", 0), ("fills_a_block", 0), ("long_at_last_thread", 255)):
        i = marks[m]
        assert head[i] % BLOCK == phase and length[i] >= 3, m
    i = marks["at_last_thread"]
    assert head[i] // BLOCK != (head[i] + length[i] - 1) // BLOCK                 # it straddles the edge
    assert marks["last"] == len(lengths) - 1 and head[-1] + length[-1] == t.n_valid and length[-1] >= 3
    assert set(RUN_LENGTHS) <= set(length.tolist())
    return t


# ---- case 7: the CSR row search ---------------------------------------------------------------------------------------------------
def rows_table(name, row_lengths, R, seed, n_drop=0, p_run=0.15):
    """A CSR table with the given entries per cell: the columns of a cell are distinct regions in random order, except for
    runs of 3 .. 6 neighbouring entries on one region (p_run of the pairs, where the row has room) and rows longer than R,
    which repeat regions; n_drop of the entries are dropped (they count in row_lengths)."""
    rng = np.random.default_rng(seed)
    row_lengths = np.asarray(row_lengths, dtype=np.int64)
    G = len(row_lengths)
    pc, pr, lengths = [], [], []
    for g in np.flatnonzero(row_lengths):
        L = draw_lengths(rng, int(row_lengths[g]), p_run)
        while len(L) > R:                                        # more pairs than regions: fold singles into longer runs
            L = np.concatenate([L[:-2], [L[-2] + L[-1]]])
        lengths.append(L)
        pc.append(np.full(len(L), g))
        pr.append(rng.choice(R, len(L), replace=False))
    pc, pr, lengths = (np.concatenate(x) if x else np.zeros(0, dtype=np.int64) for x in (pc, pr, lengths))
    t = assemble(name, G, R, pc, pr, lengths, rng, 0, "csr", row_lengths=row_lengths)
    if n_drop:                                                   # dropped entries replace single rows in place
        cell, code, w = (np.array(a) for a in t.coo())
        key = cell.astype(np.int64) * R + code
        single = np.flatnonzero(np.isin(key, (pc * R + pr)[lengths == 1]))
        hit = rng.choice(single, n_drop, replace=False)
        code[hit[::2]] = -1
        w[hit[1::2]] = np.nan
        t = Table(name, G, R, cell, code, w, row_lengths=row_lengths, n_drop=n_drop, lengths=lengths)
    np.testing.assert_array_equal(np.bincount(t.cell, minlength=G), row_lengths)
    assert (np.diff(t.cell) >= 0).all()
    return t


def row_search_table():
    """The first and the last 300 rows empty; 700 empty rows whose neighbours' entries are the last of one 256-entry block
    and the first of the next; rows of exactly 256 and 512 entries that begin at a block edge; a row that begins one entry
    before an edge."""
    rng = np.random.default_rng(7)
    lens = [0] * 300 + [256] + [0] * 700 + [256, 512, 255, 40] + rng.integers(0, 30, 200).tolist() + [0] * 300
    t = rows_table("row-search", lens, 600, 71, n_drop=30)
    rowptr = t.csr()[0]
    assert rowptr[300] == 0 and rowptr[301] == 256 and rowptr[1001] == 256 and rowptr[1002] == 512           # the empty runs
    assert (rowptr[:301] == 0).all() and (rowptr[-301:] == t.n).all()
    assert rowptr[1002] % BLOCK == 0 and rowptr[1003] - rowptr[1002] == 512 and rowptr[1003] % BLOCK == 0
    assert rowptr[1004] % BLOCK == BLOCK - 1 and rowptr[1005] - rowptr[1004] == 40                          # one before an edge
    return t


def one_row_table():
    """one row holds the whole table (G = 500, R = 3000)"""
    lens = np.zeros(500, dtype=np.int64)
    lens[250] = 4000
    return rows_table("one-row", lens, 3000, 72, n_drop=20)


def single_cell_table():
    return rows_table("G=1", [300], 50, 73, n_drop=10)


def one_entry_rows_table():
    return rows_table("one-entry-rows", [1] * 1025, 37, 74)


# ---- case 8: the one-pass partition beyond one tile, and its bins ------------------------------------------------------------------
def filled_table(R, variant="full", seed=8):
    """G = 256, every (cell, region) pair once, in (cell, region) order: 128 R pairs per chunk.  variant "edges" (R = 64):
    cell 5 has no row (chunk 0: 8128 pairs) and pair (200, 17) comes twice (chunk 1: 8193); "runs": 200 pairs carry runs of
    3 .. 6 neighbouring entries, cell 5 has no row."""
    G = 256
    rng = np.random.default_rng(seed + R)
    pc, pr = np.repeat(np.arange(G), R), np.tile(np.arange(R), G)
    lengths = np.ones(G * R, dtype=np.int64)
    if variant == "edges":
        lengths[200 * R + 17] = 2
        sel = pc != 5
        pc, pr, lengths = pc[sel], pr[sel], lengths[sel]
    elif variant == "runs":
        lengths[rng.choice(G * R, 200, replace=False)] = 3 + np.arange(200) % 4
        sel = pc != 5                                            # (cell 5 has no row here either)
        pc, pr, lengths = pc[sel], pr[sel], lengths[sel]
    t = assemble("filled-%d-%s" % (R, variant), G, R, pc, pr, lengths, rng, 0, "csr_sorted")
    rowptr = t.csr()[0]
    t.meta["chunk_pairs"] = (int(rowptr[128]), int(rowptr[256] - rowptr[128]))
    return t


def bins_table(R):
    """G = 256, R = 44,032 (64 region blocks: 1024 bins, the most the one-pass partition takes) or 44,033 (65: general
    sort): 4000 valid rows, pairs in bin 0 and in the last wave of the last region block, nothing dropped"""
    G = 256
    n_rb, rw, _ = geometry(G, R)
    must = [(0, 0), (G - 1, R - 1), (127, R - 1), (128, 0), (3, R - 2), (130, 1)]
    t = random_table("bins-%d" % R, 4000, 0, G, R, R, order="csr_sorted", must=must)
    bins = chunk_bin(t.cell, t.code, G, R)
    assert bins.min() == 0 and bins.max() == (R - 1) // rw and (R != 44032 or bins.max() == 1023)
    return t


# ---- case 9: denominators -----------------------------------------------------------------------------------------------------------
DEN_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1000)


def den_table(R):
    """G = 1000, R in 12 .. 15.  Region i < 10 holds DEN_COUNTS[i] pairs, the others a random number; region 2's two pairs
    are +x and -x (den exactly 0 in any order); weights of mixed sign, 10^uniform(-6, 6); some pairs come as two rows."""
    G = 1000
    rng = np.random.default_rng(90 + R)
    counts = list(DEN_COUNTS) + rng.integers(1, 300, R - len(DEN_COUNTS)).tolist()
    pr = np.repeat(np.arange(R), counts)
    pc = np.concatenate([rng.choice(G, c, replace=False) for c in counts])
    lengths = np.where(rng.random(len(pr)) < 0.1, 2, 1)
    lengths[pr == 2] = 1
    n = int(lengths.sum())
    w = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, 6, n)
    first = np.concatenate([[0], np.cumsum(lengths)])[:-1]
    i2 = first[pr == 2]
    w[i2[1]] = -w[i2[0]]
    t = assemble("den-%d" % R, G, R, pc, pr, lengths, rng, 40, "scattered", w=w, counts=np.array(counts), cancel_region=2)
    ref = t.ref()
    np.testing.assert_array_equal(ref.n_r, counts)
    assert ref.den[2] == 0.0 and (ref.den[np.arange(R) != 2][np.array(counts)[np.arange(R) != 2] > 0] != 0).all()
    return t


# ---- tables without repeated pairs (any row order gives the same plan) ----------------------------------------------------------------
def distinct_table(n=20000, G=300, R=100, seed=11):
    return random_table("distinct-%d" % n, n, 150, G, R, seed, p_run=0.0)


def permuted(t, how, seed=0):
    o = np.arange(t.n)[::-1] if how == "reversed" else np.random.default_rng(seed).permutation(t.n)
    return Table(t.name + "-" + how, t.G, t.R, t.cell[o], t.code[o], t.w[o])


# ---- case 10: refusals ------------------------------------------------------------------------------------------------------------
def bad_rows_table(first, others, n=20000, G=300, R=37):
    """a table whose rows `first` < `others` are out of range in turn: code >= R, cell >= G, cell < 0"""
    t = random_table("bad", n, 0, G, R, first)
    cell, code, w = (np.array(a) for a in t.coo())
    for k, i in enumerate([first] + list(others)):
        if k % 3 == 0:
            code[i] = R + k
        elif k % 3 == 1:
            cell[i] = G
        else:
            cell[i] = -1 - k
    return cell, code, w


# ---- mutations of a table (the sensitivity demonstrations of the host test) ---------------------------------------------------------
def rows_of_run(t, i):
    """the rows of the pair of run i, in table order"""
    return np.flatnonzero((t.cell == t.meta["pair_cell"][i]) & (t.code == t.meta["pair_region"][i]) & t.keep)


def mutate(t, what, run=None):
    """(cell, code, w) of the table with one defect of a builder put into the reference's input:
    "swap"   two neighbouring rows of a run exchanged, at a place where that shows
    "drop"   the last row of the run lost
    "move"   the run's pair (all its rows) in the neighbouring region
    "split"  the run's last row on a pair of its own (nnz + 1)"""
    cell, code, w = (np.array(a) for a in t.coo())
    L = t.meta["lengths"]
    if run is None:
        run = int(np.flatnonzero((L >= 4) & (L <= 6))[0])
    rows = rows_of_run(t, run)
    if what == "swap":
        i = detectable_swaps(w[rows])[-1]
        w[rows[i]], w[rows[i + 1]] = w[rows[i + 1]], w[rows[i]]
    elif what == "drop":
        code[rows[-1]] = -1
    elif what == "move":
        r = int(code[rows[0]])
        code[rows] = r + 1 if r + 1 < t.R else r - 1
    elif what == "split":
        used = set((cell[t.keep].astype(np.int64) * t.R + code[t.keep]).tolist())
        c = next(c for c in range(t.G) if c * t.R + int(code[rows[0]]) not in used)
        cell[rows[-1]] = c
    else:
        raise ValueError(what)
    return cell, code, w
