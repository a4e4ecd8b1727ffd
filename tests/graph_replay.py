"""The case table of the graph capture-and-replay tests (no test functions, no GPU needed to import or to evaluate the host side):
one or more cases per engine call that docs/STREAM_CAPTURE.md lists as capturable (DESIGN.md points there).  tests/test_graph_replay_host.py
ties this table to that list and proves that the mutations below change every case's expected result from one step to the next;
tests/test_gpu_graph_replay.py captures every case once and replays it over the mutations.

A case holds: ``build(dtype)`` -> :class:`Inputs` (host fields, the host parameter arrays of the call, the sites of the special
values), ``setup(torch, inp)`` -> what lives on the device beside the fields (plans, row lists), ``call(ctx, F, out, stream,
params)`` -> ``(result, status word or None)``, ``expect(inp, fields)`` -> the NumPy restatement of the result and
``compare(inp, got, want, fields, skip)`` -> the comparison its small-shape module makes (the restatements and tolerances are
imported from those modules; ``skip``: on the +inf step, the row / column of the result that holds the +inf -- the MFMA forms and
the row-list families leave it unspecified, every other one is checked).

MUTATIONS, applied in this order to the same device tensors: half the values; a fresh seeded field; NaN in one referenced cell and
in one whole row; +inf in one referenced, in-season cell; the clean data again."""
import collections

import numpy as np

from tests import element_ops as E
from tests import exposure_ref as ER
from tests import rowlist_layout as RL
from tests.quantile_ref import quantile_ref
from tests.rolling_ref import rolling_ref
from tests.spell_ref import in_season, spell_ref
from tests.test_gpu_bins import _restate
from tests.test_gpu_dense_forms_small import BK as DENSE_BK, EDD_THRESHOLDS, LONG, OFFSET, _oracle_of, price, priced_ok, table
from tests.test_gpu_dense_forms_small import pack_free as dense_pack_free
from tests.test_gpu_hinge import _terms
from tests.test_gpu_packed_totals import _Sparse
from tests.test_gpu_parity import RTOL32, RTOL64, _rel_ok
from tests.test_gpu_periods import _psum
from tests.test_gpu_rolling import RB2, ROWS2, T2

F32, F64 = np.float32, np.float64
BOTH = (F32, F64)
RTOL = {F32: RTOL32, F64: RTOL64}
KELVIN = RL.KELVIN
MUTATIONS = ("half", "fresh", "nan", "inf", "clean")
STATUS_POISON = 0x5A5A5A

# the two-period lists of tests/test_gpu_rolling.py (33 + 4 rows of T = 40; rows 0, 1 and 35 are in no list), and the same with an
# empty third period.  With two periods a splitting family cuts each list into two parts (37 // 2 // 8 = 2); the empty period makes
# the mean list shorter than two parts' worth, so those lists go to the families that never split
RL.LISTS.setdefault("replay", (T2, RB2, ROWS2))
RL.LISTS.setdefault("replay_empty", (T2, np.concatenate([RB2, RB2[-1:]]), ROWS2))
RL_NS = (5, 1029)                                        # VEC = 1 | crosses a column block on 16-byte loads

Inputs = collections.namedtuple("Inputs", "dtype fields params nan_cell nan_row inf_at skip aux")


class Case:
    def __init__(self, name, label, dtypes, build, fresh, setup, call, expect, compare, warmups=1, status="none"):
        self.name, self.label, self.dtypes = name, label, dtypes
        self.build, self.fresh, self.setup, self.call, self.expect, self.compare = build, fresh, setup, call, expect, compare
        self.warmups = warmups
        self.takes_out = True                            # does the call take ``out=``?
        self.out_dtype = None                            # the result's element type where it is not the fields'
        self.status = status                             # "none" | "word": a status tensor the call zero-fills | "saw_inf": DensePlan's note

    @property
    def id(self):
        return "%s[%s]" % (self.name, self.label)


def steps(case, inp):
    """[(mutation, host fields)] in the order of MUTATIONS"""
    clean = [np.array(f) for f in inp.fields]
    half = [(f * f.dtype.type(0.5)).astype(f.dtype) for f in clean]
    fresh = [np.array(f) for f in case.fresh(inp)]
    nan = [f.copy() for f in fresh]
    nan[0][inp.nan_cell] = np.nan
    for f in nan:
        f[inp.nan_row] = np.nan
    inf = [f.copy() for f in nan]
    for f in inf:
        f[inp.inf_at] = np.inf
    return list(zip(MUTATIONS, (half, fresh, nan, inf, clean)))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view({4: np.uint32, 8: np.uint64}[a.itemsize])


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert len(bad) == 0, "%s: %d of %d elements differ in their bits, first at flat index %d: got %r, want %r" % (
        what, len(bad), got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def _drop(a, skip, axes):
    """``a`` without index skip[1] of the axis that ``skip[0]`` ("row" / "col") names in ``axes``"""
    return a if skip is None else np.delete(a, skip[1], axis=axes[skip[0]])


def _dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _i32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def pick_ksplit(items, n_kt):
    """csrc/wagg_dense_route.cpp: pick_ksplit restated -- multiples of 8, at least 32 k tiles a slice beyond 8, the best fill of 256 CUs"""
    best, best_eff = 8, 0.0
    for S in range(8, 65, 8):
        if S > 8 and n_kt // S < 32:
            break
        w = items * S / 256.0
        eff = w / np.ceil(w)
        if eff > best_eff + 1e-9:
            best_eff, best = eff, S
        if eff >= 0.985:
            break
    return best


def n_row_blocks(T, dtype):
    """row blocks of one launch group: at most 23 (fp32) / 11 (fp64) sixteen-row units each"""
    return -(-T // (16 * (23 if dtype == F32 else 11)))


# ---- dense-family plans -----------------------------------------------------------------------------------------------------------
def _dense_field(G, R, dtype, T, seed, nan=True):
    """tests/test_gpu_dense_forms_small.py's kelvin_field with a seed: the region whose weights cancel keeps a numerator of one sign.
    ``nan=False``: no NaN anywhere -- the plain applies, so that a plan is clean up to the capture and the graph holds the
    pack-free first pass, the zero-fill of the gate word and the gated second pass where the route has them"""
    t = table(G, R)
    rng = np.random.default_rng(31 * G + T + 977 * seed)
    X = (-OFFSET + 22 + 8 * rng.standard_normal((T, G))).astype(dtype)
    X[:, t.c_sum0[0]] = X[:, t.c_sum0[1]] + dtype(10)
    if nan:
        X[4, 100:103] = np.nan
    return X


def _dense_edd_pair(G, R, dtype, T, seed):
    """that module's edd_fields with a seed (degrees C, tasmin <= tasmax)"""
    t = table(G, R)
    rng = np.random.default_rng(37 * G + T + 977 * seed)
    mean, half = 22 + 8 * rng.standard_normal((T, G)), rng.uniform(0, 8, (T, G))
    lo, hi = (mean - half).astype(dtype), (mean + half).astype(dtype)
    hi = np.maximum(lo, hi)
    lo[:, t.c_sum0[0]], hi[:, t.c_sum0[0]] = 24, 34
    lo[:, t.c_sum0[1]], hi[:, t.c_sum0[1]] = 12, 18
    lo[6, 90:93] = np.nan
    hi[8, 110:113] = np.nan
    return lo, hi


def _dense_case(kind, G, R, form, variant, T, dtypes, ksplit=0):
    from oracle import ref_numpy as O
    split, exact = variant == "split", variant == "exact"
    # cell 0 holds a pair in every table; row 9: +inf, row 11: NaN throughout, (13, 0): one NaN
    sites = dict(nan_cell=(13, 0), nan_row=11, inf_at=(9, 0), skip=("row", 9))

    def fields(dtype, seed):
        return list(_dense_edd_pair(G, R, dtype, T, seed)) if kind == "edd" else [_dense_field(G, R, dtype, T, seed, nan=kind != "apply")]

    def build(dtype):
        return Inputs(dtype, fields(dtype, 0), {}, aux=None, **sites)

    def setup(torch, inp):
        from tests.test_gpu_dense_forms_small import build_plan
        plan = build_plan(G, R, form, inp.dtype)
        if split:
            assert plan.info["w_image_bytes"] > 0, "the split form is to run with the W image on"
        return plan

    def call(plan, F, out, stream, params):
        if kind == "apply":
            return plan.apply(F[0], out=out, ksplit=ksplit, stream=stream, exact=exact), None
        if kind == "poly":
            return plan.apply_poly(F[0], OFFSET, 2, out=out, stream=stream, exact=exact), None
        return plan.apply_edd(F[0], F[1], EDD_THRESHOLDS[1], out=out, stream=stream, exact=exact), None

    def transformed(F):
        if kind == "apply":
            return F[0]
        return O.tas_poly_values(F[0], 2, OFFSET) if kind == "poly" else O.snyder_edd_values(F[0], F[1], EDD_THRESHOLDS[1])

    def expect(inp, F):
        return _oracle_of(transformed(F), G, R)

    def compare(inp, got, want, F, skip):
        axes = {"row": 0}
        if kind == "apply":
            priced_ok(_drop(got, skip, axes), _drop(want, skip, axes), _drop(price(F[0], G, R, inp.dtype, split=split), skip, axes))
        else:
            _rel_ok(_drop(got, skip, axes), _drop(want, skip, axes), RTOL[inp.dtype], scale=100.0 if kind == "poly" else 0.05)

    name = {"apply": "DensePlan.apply", "poly": "DensePlan.apply_poly", "edd": "DensePlan.apply_edd"}[kind]
    label = "%s%s %dx%d T%d%s" % (form, "-" + variant if variant else "", G, R, T, " ksplit %d" % ksplit if ksplit else "")
    case = Case(name, label, dtypes, build, lambda inp: fields(inp.dtype, 1), setup, call, expect, compare,
                warmups=2 if split else 1, status="none" if form == "entries" else "saw_inf")
    # does the captured apply start with a pack-free pass?  (the route of a clean plan on 16-byte aligned, contiguous rows)
    case.pack_free = {dt: kind == "apply" and dense_pack_free(G, dt, form, variant, T, True) for dt in dtypes}
    # the k slices of the launch: the caller's, else the library's choice (csrc/wagg_dense_route.cpp: pick_ksplit), 1 for tiles
    case.k_slices = {dt: None if form == "entries" else 1 if form == "tiles" else ksplit or pick_ksplit(-(-R // 256) * n_row_blocks(T, dt), -(-G // DENSE_BK[dt]))
                     for dt in dtypes}
    return case


# ---- segment-table plans ----------------------------------------------------------------------------------------------------------
def _sparse(dtype, seed=5):
    return _Sparse(16, 32, dtype, seed=seed)


class _RouteGrid:
    """A grid and table of tests/test_gpu_fallback_routes.py with the attributes of _Sparse; ``plan()`` is the DEFAULT plan (row_len
    given, no flags): whole-line chunkings where nlon is a multiple of 4 (``info["lines"] == 7``), the region-shaped routes on the
    ragged 37 x 27 grid -- what csrc/wagg_route.cpp selects without an override; every table carries a giant region"""

    def __init__(self, grid, T, dtype, seed):
        import pandas as pd
        from tests.test_gpu_fallback_routes import _table
        t = _table(*grid)
        self.t, self.grid, self.T, self.G, self.R, self.nlon, self.dtype = t, grid, T, t.G, t.R, t.nlon, dtype
        self.cell, self.code, self.w_eff = t.cell, t.code, t.w
        self.df = pd.DataFrame({"areawt": np.where(np.isnan(t.w), 1.0, np.abs(t.w) + 0.5)})
        rng = np.random.default_rng(1000 + T + 977 * seed)
        tas = (-OFFSET + 22 + 8 * rng.standard_normal((T, t.G))).astype(dtype)
        tas[:, t.c["a"]] = tas[:, t.c["b"]] + dtype(10)              # (the numerator of the region whose weights sum to 0 keeps its sign)
        self.tas, self.tasmax = tas, (tas + rng.uniform(0, 12, tas.shape)).astype(dtype)
        self.sites = (int(t.c["nan"]), int(t.c["pinf"]))             # the +inf cell: weight > 0 in its block region, 0 in its sibling

    def plan(self):
        from climate_toolbox_amd.engine import SparsePlan
        p = SparsePlan(self.cell, self.code, self.w_eff, self.G, self.R, row_len=self.nlon)
        assert p.info["n_giant"] >= 1 and p.info["lines"] == (7 if self.nlon % 4 == 0 else 0), (self.grid, p.info["lines"], p.info["n_giant"])
        return p


def _sparse_fields(c, two):
    return [np.array(f).reshape(c.T, c.G) for f in ((c.tas, c.tasmax) if two else (c.tas,))]


def _many_plan(c):
    from climate_toolbox_amd import engine
    return engine.ManyPlan(c.cell, c.code, [c.w_eff, c.df["areawt"].to_numpy()], c.G, c.R, row_len=c.nlon, levels=[(c.code // 4, (c.R + 3) // 4)])


def _sparse_case(kind, grid=None, T=None):
    from oracle import ref_numpy as O
    two = kind == "edd"
    thr = [285.0, 290.0]

    def make(dtype, seed):
        return _sparse(dtype, seed) if grid is None else _RouteGrid(grid, T, dtype, seed)

    def build(dtype):
        c = make(dtype, 5)
        g, gi = (int(c.cell[0]),) * 2 if grid is None else c.sites     # referenced cells
        return Inputs(dtype, _sparse_fields(c, two), {"thr": np.array(thr)} if two else {}, (7, g), 21, (30, gi), ("row", 30), c)

    def setup(torch, inp):
        return _many_plan(inp.aux) if kind == "many" else inp.aux.plan()

    def call(plan, F, out, stream, params):
        if kind == "apply":
            return plan.apply(F[0], out=out, stream=stream), None
        if kind == "rt":
            return plan.apply(F[0], out=out, out_layout="RT", stream=stream), None
        if kind == "compact":                            # the rows packed by pack_rows, then contracted: two calls, one stream
            from climate_toolbox_amd import engine
            return plan.apply(engine.pack_rows(plan, F[0], stream=stream), out=out, compact=True, stream=stream), None
        if kind == "poly":
            return plan.apply_poly(F[0], KELVIN, 3, out=out, stream=stream), None
        if kind == "edd":
            return plan.apply_edd(F[0], F[1], params["thr"], out=out, stream=stream), None
        if out is None:
            out = F[0].new_empty((F[0].shape[0], plan.out_cols))
        plan.apply(F[0], out=out, stream=stream)
        return out, None

    def expect(inp, F):
        c = inp.aux
        agg = lambda X, code=c.code, w=c.w_eff, R=c.R: O.agg_coded(X, c.cell, code, w, R)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if kind in ("apply", "compact"):
                return agg(F[0])
            if kind == "rt":
                return np.ascontiguousarray(agg(F[0]).T)
            if kind == "poly":
                return np.stack([agg(O.tas_poly_values(F[0], p, KELVIN)) for p in (1, 2, 3)])
            if kind == "edd":
                return np.stack([agg(O.snyder_edd_values(F[0], F[1], e)) for e in thr])
            ws = [c.w_eff, c.df["areawt"].to_numpy()]
            return np.concatenate([agg(F[0], w=w) for w in ws] + [agg(F[0], code=c.code // 4, w=w, R=(c.R + 3) // 4) for w in ws], axis=1)

    def compare(inp, got, want, F, skip):
        axes = {"row": {"apply": 0, "compact": 0, "rt": 1, "poly": 1, "edd": 1, "many": 0}[kind]}
        got, want = _drop(got, skip, axes), _drop(want, skip, axes)
        if kind == "poly":
            for k in range(3):
                _rel_ok(got[k], want[k], RTOL[inp.dtype], scale=10.0 ** (k + 1))
        else:
            _rel_ok(got, want, RTOL[inp.dtype], scale=0.05 if kind == "edd" else None)

    name = {"apply": "SparsePlan.apply", "rt": "SparsePlan.apply", "compact": "SparsePlan.apply", "poly": "SparsePlan.apply_poly", "edd": "SparsePlan.apply_edd",
            "many": "ManyPlan.apply"}[kind]
    label = {"apply": "TR", "rt": "RT", "compact": "compact rows from pack_rows", "poly": "three powers", "edd": "two thresholds", "many": "two weightings, two levels"}[kind]
    if grid is not None:
        label = "%dx%d T%d %s" % (grid[0], grid[1], T, label)
    return Case(name, label, BOTH, build, lambda inp: _sparse_fields(make(inp.dtype, 6), two), setup, call, expect, compare)


# ---- the row-list families --------------------------------------------------------------------------------------------------------
RL_VARIANTS = {
    "period": RL.Variant("poly", False, 3, None), "season": RL.Variant("poly", False, 3, None),
    "edd_ladder": RL.FAMILIES["edd_ladder"].variants[0], "bin_days": RL.FAMILIES["bin_days"].variants[0],
    "hinge": RL.FAMILIES["hinge"].variants[0], "exposure": RL.FAMILIES["exposure"].variants[0],
    "spell": RL.Variant("days1-above", False, 3, (1, "days", "above")),         # every hot day counts: one +inf day is one more
    "rolling": RL.FAMILIES["rolling"].variants[0], "quantile": RL.Variant("linear-q8", False, 8, ("linear", RL.Q8, 33)),
}
RL_ENGINE = {"period": "period_reduce", "season": "season_reduce", "edd_ladder": "edd_ladder_reduce", "bin_days": "bin_days_reduce",
             "hinge": "hinge_reduce", "exposure": "exposure_reduce", "spell": "spell_reduce", "rolling": "rolling_reduce",
             "quantile": "quantile_select"}


def rl_expect(name, d, v):
    """The (planes, P, n) restatement of family ``name`` on Data ``d``: what its check in tests/rowlist_layout.py compares with"""
    from oracle import ref_numpy as O
    sk = (d.doy, d.win) if d.seasoned else (None, None)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if name in ("period", "season"):
            return np.stack([_psum(d.m01 * np.nan_to_num(O.tas_poly_values(d.X, k + 1), nan=0.0), d.rb, d.rows) for k in range(v.planes)])
        if name == "edd_ladder":
            cmin, cmax = d.X + d.dtype(KELVIN), d.H + d.dtype(KELVIN)
            return np.stack([_psum(d.m01 * np.nan_to_num(O.snyder_edd_values(cmin, cmax, e), nan=0.0), d.rb, d.rows) for e in v.p])
        if name == "bin_days":
            return _restate(d.X, d.m01, d.rb, d.rows, v.p, KELVIN)
        if name == "hinge":
            return np.stack([_psum(p * d.m01, d.rb, d.rows) for p in _terms(d.X, KELVIN, np.asarray(RL.KNOTS9), v.p[0], v.p[1])])
        if name == "exposure":
            return ER.exposure_bins(d.X, d.H, KELVIN, v.p, d.rb, d.rows, d.m01)
        if name == "spell":
            return spell_ref(d.X, d.rb, d.rows, KELVIN, RL.SPELL_THR, v.p[0], v.p[1], v.p[2], *sk)
        if name == "rolling":
            return rolling_ref(d.X, d.rb, d.rows, KELVIN, v.p[0], v.p[1], v.p[2], *sk)
        return quantile_ref(d.X, d.rb, d.rows, KELVIN, v.p[1], v.p[0], *sk)


def rl_full_work(L, fam, v, d):
    return RL.full_work_bytes(L, fam, v, d.n, d.P, len(d.rows)) if fam.splits else 0


def rl_split(L, name, d, v):
    """the parts the library cuts a list into for this case, by tests/rowlist_layout.py's restatement of its rule"""
    fam = RL.FAMILIES[name]
    if not fam.splits:
        return 1
    vcells = RL.vec(d.dtype) if rl_pitch(d.n, d.dtype) % RL.vec(d.dtype) == 0 else 1      # (the fields start on 16 bytes)
    return RL.expected_split("full", rl_full_work(L, fam, v, d), v.planes, d.P, d.n, len(d.rows), vcells)


def rl_pitch(n, dtype):
    """the row pitch of a row-list case's fields: n = 5 contiguous (one cell per lane), n = 1029 on the next multiple of a
    16-byte piece (route "1" of tests/rowlist_layout.py: 16-byte loads, two column blocks)"""
    return n if n == 5 else RL.ldx_for("1", n, dtype)


def _rl_case(name, n, lists=None, own_status=False):
    fam, v = RL.FAMILIES[name], RL_VARIANTS[name]
    seasoned = RL.seasoned_for(fam, n != 5)                          # n = 5 without a season where the family has the choice
    lists = lists or ("replay" if fam.splits else "replay_empty")

    def data(dtype, seed):
        return RL.make_data(lists, n, dtype, seasoned, seed=seed)

    def with_fields(d, F):
        return d._replace(X=F[0], H=F[1])

    def build(dtype):
        d = data(dtype, 0)
        f = data(dtype, 1)
        listed = np.zeros(d.T, dtype=bool)
        listed[d.rows[d.rb[0]:d.rb[1]]] = True                       # the long period's rows
        ok = listed[:, None] & (d.m01 > 0) & np.isfinite(f.X) & np.isfinite(f.H) & ~np.isin(np.arange(n), (2, 3, 6))[None, :]
        whole = int(np.argmax(np.where(listed, (d.m01 > 0).sum(1), -1)))   # the listed row most cells are in season on: NaN throughout
        ok[whole] = False
        every = np.zeros(d.T, dtype=bool)
        every[d.rows] = True
        cand = np.argwhere(ok)
        for r, c in cand[np.argsort(f.X[ok], kind="stable")]:        # the coldest such cell of the fresh field: +inf there is news
            r, c = int(r), int(c)
            ok2 = every[:, None] & (d.m01 > 0) & np.isfinite(f.X) & np.isfinite(f.H) & ~np.isin(np.arange(n), (2, 3, c))[None, :]
            ok2[whole] = False
            if ok2.any():                                            # (a column of its own for the single NaN)
                break
        if not ok2.any():                                            # one cell in season only: the NaN shares the +inf cell's column
            ok2 = ok.copy()
            ok2[r] = False
        others = np.argwhere(ok2)
        nr, nc = (int(x) for x in others[np.argmax(f.X[ok2])])       # the hottest one: a NaN there lowers a one-day maximum
        return Inputs(dtype, [d.X, d.H], _params(), (nr, nc), whole, (r, c), ("col", c), d)

    def _params():
        p = v.p
        if name in ("period", "season"):
            return {}
        if name == "hinge":
            return {"list": np.array(RL.KNOTS9, dtype=np.float64)}
        if name == "spell":
            return {"list": np.array(RL.SPELL_THR, dtype=np.float64)}
        if name == "rolling":
            return {"list": np.array(p[0], dtype=np.int64)}
        if name == "quantile":
            return {"list": np.array(p[1], dtype=np.float64)}
        return {"list": np.array(p, dtype=np.float64)}

    def setup(torch, inp):
        from climate_toolbox_amd import engine
        d = inp.aux
        rb, rw = engine.period_lists(d.rb, d.rows, d.T)
        return dict(rb=rb, rw=rw, doy=_i32(torch, d.doy), win=_i32(torch, d.win), status=torch.zeros(1, dtype=torch.int32, device="cuda"))

    def call(ctx, F, out, stream, params):
        from climate_toolbox_amd import engine
        kw = dict(checked=True, out=out, stream=stream)
        if own_status:                                               # the caller's status word (the caller resets it) and no workspace
            kw.update(status=ctx["status"], workspace=False)
        sk = dict(doy=ctx["doy"], windows=ctx["win"]) if seasoned else {}
        rb, rw, p = ctx["rb"], ctx["rw"], v.p
        if name == "period":
            return engine.period_reduce(F[0], rb, rw, poly=(KELVIN, 1, v.planes), **kw)
        if name == "season":
            return engine.season_reduce(F[0], rb, rw, ctx["doy"], ctx["win"], poly=(KELVIN, 1, v.planes), **kw)
        lst = params["list"]
        if name == "edd_ladder":
            return engine.edd_ladder_reduce(F[0], F[1], rb, rw, KELVIN, lst, **sk, **kw)
        if name == "exposure":
            return engine.exposure_reduce(F[0], F[1], rb, rw, KELVIN, lst, **sk, **kw)
        if name == "bin_days":
            return engine.bin_days_reduce(F[0], rb, rw, KELVIN, lst, **sk, **kw)
        if name == "hinge":
            return engine.hinge_reduce(F[0], rb, rw, KELVIN, lst, power=p[0], side=p[1], **sk, **kw)
        if name == "spell":
            return engine.spell_reduce(F[0], rb, rw, KELVIN, lst, min_length=p[0], stat=p[1], side=p[2], **sk, **kw)
        if name == "rolling":
            return engine.rolling_reduce(F[0], rb, rw, KELVIN, [int(w) for w in lst], stat=p[1], of=p[2], **sk, **kw)
        return engine.quantile_select(F[0], rb, rw, KELVIN, lst, method=p[0], max_rows=p[2], **sk, **kw)

    def expect(inp, F):
        return rl_expect(name, with_fields(inp.aux, F), v)

    def compare(inp, got, want, F, skip):
        d = with_fields(inp.aux, F)
        if skip is not None:                                         # the +inf cell's column: unspecified sums, left out of the check --
            c, c2 = skip[1], 1 if skip[1] == 0 else 0                # column c2 stands in for it, in the data and in the result
            X, H, m01, win, got = (np.array(a) for a in (d.X, d.H, d.m01, d.win, got))
            X[:, c], H[:, c], m01[:, c], win[c], got[:, :, c] = X[:, c2], H[:, c2], m01[:, c2], win[c2], got[:, :, c2]
            d = d._replace(X=X, H=H, m01=m01, win=win)
        if name == "exposure":                                       # its module's tolerance, RTOL x the counted days, without the
            want = ER.exposure_bins(d.X, d.H, KELVIN, v.p, d.rb, d.rows, d.m01)       # claims about that module's own clean data
            D = ER.counted_days(d.X, d.H, d.rb, d.rows, d.m01)
            g = np.asarray(got, dtype=np.float64)
            assert np.isfinite(g).all()
            bad = np.argwhere(np.abs(g - want) > RTOL[d.dtype] * D[None])
            assert len(bad) == 0, "exposure: %d values beyond tol * D, first at (bin, period, cell) %r" % (len(bad), tuple(bad[0]))
            return
        fam.check(got, d, v)

    label = "n%d %s%s%s" % (n, "season" if seasoned else "no season", " empty period" if lists == "replay_empty" and fam.splits else "",
                            " own status" if own_status else "")
    case = Case(RL_ENGINE[name], label, BOTH, build,
                lambda inp: [data(inp.dtype, 1).X, data(inp.dtype, 1).H], setup, call, expect, compare, status="own word" if own_status else "word")
    case.family, case.variant, case.pitch = name, v, rl_pitch
    case.parts = 1 if own_status or lists == "replay_empty" or not fam.splits else 2
    return case


# ---- element and data-movement calls ----------------------------------------------------------------------------------------------
EL_T, EL_N = 23, 257                                                 # tests/test_gpu_element_ops.py's gather / stream-order shape


def _el_field(dtype, seed, hi=False):
    rng = np.random.default_rng(900 + seed)
    lo = (280 + 15 * rng.standard_normal((EL_T, EL_N))).astype(dtype)
    return [lo, (lo + rng.uniform(0.0, 12.0, lo.shape)).astype(dtype)] if hi else [lo]


def _el_case(name, label, call, ref, exact=True, hi=False, params=None, tol=None, setup=None, dtypes=BOTH, skip_inf=False):
    """``skip_inf``: the element that holds the +inf is left out of the comparison with the restatement (transform_edd: the
    reference's expression is inf - inf there)"""
    inf_at = (17, int(EL_IDX[0]))

    def build(dtype):
        return Inputs(dtype, _el_field(dtype, 0, hi), {} if params is None else params(), (5, int(EL_IDX[1])), 12, inf_at,
                      ("elem", inf_at) if skip_inf else None, None)

    def compare(inp, got, want, F, skip):
        if exact:
            same_bits(got, want.astype(got.dtype), name)
            return
        if skip is not None:
            got, want = np.array(got), np.array(want)
            got[skip[1]], want[skip[1]] = 0, 0
        tol(inp, got, want, F)

    case = Case(name, label, dtypes, build, lambda inp: _el_field(inp.dtype, 1, hi), setup or (lambda torch, inp: None), call,
                lambda inp, F: ref(inp, F), compare)
    case.takes_out, case.out_dtype = False, F64 if name == "to_float64" else None
    return case


EL_IDX = np.random.default_rng(2).integers(0, EL_N, 100)
EDD_TERMS = [(1.0, 10.0), (-1.0, 30.0)]
COMBINE = [1.0, -2.0, 0.25]


def _edd_terms_ref(inp, F):
    from oracle import ref_numpy as O
    ft = inp.dtype
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = F[0] + ft(KELVIN), F[1] + ft(KELVIN)
        return sum(c * O.snyder_edd_values(lo, hi, e).astype(np.float64) for c, e in EDD_TERMS)


def _edd_terms_tol(inp, got, want, F):
    _rel_ok(got, want, RTOL[inp.dtype], scale=0.05)


def _combine_ref(inp, F):
    planes = np.stack([F[0], F[1], F[0] * inp.dtype(0.5)]).reshape(3, -1)
    return E.combine_ref(planes, COMBINE)[0].reshape(F[0].shape)


def _combine_tol(inp, got, want, F):
    planes = np.stack([F[0], F[1], F[0] * inp.dtype(0.5)]).reshape(3, -1)
    ref, S = E.combine_ref(planes, COMBINE)
    fin = np.isfinite(ref)
    g = got.reshape(-1)
    np.testing.assert_array_equal(np.isnan(g), np.isnan(ref))
    np.testing.assert_array_equal(g[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)].astype(g.dtype))
    err = np.abs(g[fin].astype(ref.dtype) - ref[fin]).astype(np.float64)
    assert (err <= np.asarray(E.combine_bound(3, S, inp.dtype))[fin]).all(), "combine_planes beyond K eps S"


def _season_mask_case():
    """no floating-point operand: the mutations act on the day-of-year vector and the windows instead"""
    T, n = 40, 257
    doy0 = np.arange(100, 100 + T).astype(np.int32)
    win0 = np.where(np.arange(n) % 3 == 0, 0 | 1023 << 10, 101 | 112 << 10).astype(np.int32)

    def build(dtype):
        return Inputs(dtype, [doy0.reshape(1, T), win0.reshape(1, n)], {}, None, None, None, None, None)

    def ref(inp, F):
        doy, win = F[0].reshape(-1), F[1].reshape(-1)
        m = np.stack([in_season(int(d), win) for d in doy]).astype(np.float64).T
        m[(win & (1 << 21)) != 0] = np.nan
        return np.ascontiguousarray(m)

    case = Case("season_mask", "device vectors", (F64,), build, None, lambda torch, inp: None,
                lambda ctx, F, out, stream, params: (_engine().season_mask(F[0].reshape(-1), F[1].reshape(-1), stream=stream), None),
                ref, lambda inp, got, want, F, skip: same_bits(got, want, "season_mask"))

    case.takes_out, case.out_dtype = False, F64

    def own_steps(inp):
        doy, win = inp.fields
        half = [doy // 2 + 52, win]
        fresh = [(doy + 7).astype(np.int32), np.roll(win, 1)]
        nan = [fresh[0].copy(), fresh[1].copy()]
        nan[1][0, 5] |= 1 << 21                                      # a null window: NaN throughout that cell
        nan[0][0, 12] = 2000                                         # a day in no season: 0 throughout that row
        inf = [nan[0].copy(), nan[1].copy()]
        inf[1][0, 7] ^= 1 << 20                                      # one window inverted
        return list(zip(MUTATIONS, (half, fresh, nan, inf, [doy, win])))
    case.own_steps = own_steps
    return case


def _pack_case(two):
    def cells_of(c):
        q = np.unique(c.cell // 4)
        return (4 * q[:, None] + np.arange(4)[None, :]).reshape(-1)

    def build(dtype):
        c = _sparse(dtype)
        g = int(c.cell[0])
        return Inputs(dtype, _sparse_fields(c, two), {}, (7, g), 21, (30, g), None, c)

    def ref(inp, F):
        cells = getattr(inp.aux, "compact", None)        # the plan's own order of the referenced quads, once there is a plan
        cells = cells_of(inp.aux) if cells is None else cells
        return np.concatenate([f[:, cells] for f in F], axis=1)

    def setup(torch, inp):
        plan = inp.aux.plan()
        inp.aux.compact = np.array(plan.compact_cells(inp.dtype))
        q = inp.aux.compact.reshape(-1, 4)
        assert (q[:, 0] % 4 == 0).all() and (q == q[:, :1] + np.arange(4)).all() and int(inp.aux.cell[0]) in inp.aux.compact, "whole quads"
        return plan

    def call(plan, F, out, stream, params):
        from climate_toolbox_amd import engine
        return engine.pack_rows(plan, F[0], F[1] if two else None, stream=stream), None

    case = Case("pack_rows", "two fields" if two else "one field", BOTH, build, lambda inp: _sparse_fields(_sparse(inp.dtype, seed=6), two),
                setup, call, ref, lambda inp, got, want, F, skip: same_bits(got, want.astype(got.dtype), "pack_rows"))
    case.takes_out = False
    return case


def _engine():
    from climate_toolbox_amd import engine
    return engine


def _build_cases():
    cases = [
        _dense_case("apply", 129, 17, "full", "split", 65, (F32,)),
        _dense_case("apply", 384, 689, "full", "exact", 640, (F32,)),        # the pack-free pass and its gated second pass
        _dense_case("apply", 384, 689, "full", "", 320, (F64,)),
        _dense_case("apply", 385, 688, "full", "split", 65, (F32,)),
        _dense_case("apply", 385, 688, "full", "split", 65, (F32,), ksplit=16),      # 13 k tiles in 16 slices: a caller's k-split
        _dense_case("apply", 385, 688, "full", "", 65, (F64,)),               # one packed T
        _dense_case("apply", 129, 17, "tiles", "", 65, BOTH),
        _dense_case("apply", 384, 689, "tiles", "", 65, BOTH),               # tile-sparse, pack-free
        _dense_case("apply", LONG[0], LONG[1], "entries", "", 65, BOTH),
        _dense_case("poly", 129, 17, "full", "split", 65, (F32,)),
        _dense_case("poly", 129, 17, "full", "", 65, (F64,)),
        _dense_case("poly", LONG[0], LONG[1], "entries", "", 65, BOTH),
        _dense_case("edd", 129, 17, "full", "split", 65, (F32,)),
        _dense_case("edd", 129, 17, "tiles", "", 65, (F64,)),
        _sparse_case("apply", (40, 36), 130), _sparse_case("apply", (61, 100), 65), _sparse_case("apply", (96, 192), 64),
        _sparse_case("apply", (37, 27), 63), _sparse_case("poly", (37, 27), 63), _sparse_case("edd", (37, 27), 63),
        _sparse_case("edd", (40, 36), 130), _sparse_case("many", (61, 100), 65),      # (derived levels need a whole-line chunking: not the ragged grid)
        _sparse_case("apply"), _sparse_case("rt"), _sparse_case("compact"), _sparse_case("poly"), _sparse_case("edd"), _sparse_case("many"),
    ]
    cases += [_rl_case(name, n) for name in RL_ENGINE for n in RL_NS]
    cases += [_rl_case(name, 1029, lists="replay_empty") for name in RL_ENGINE if RL.FAMILIES[name].splits]
    cases += [_rl_case("period", 1029, own_status=True), _rl_case("hinge", 5, own_status=True)]
    e = _engine
    cases += [
        _season_mask_case(),
        _el_case("gather", "TG -> TR", lambda ctx, F, out, s, p: (e().gather(F[0], ctx, stream=s), None),
                 lambda inp, F: F[0][:, EL_IDX], setup=lambda torch, inp: _i32(torch, EL_IDX)),
        _el_case("gather", "TG -> RT", lambda ctx, F, out, s, p: (e().gather(F[0], ctx, out_layout="RT", stream=s), None),
                 lambda inp, F: np.ascontiguousarray(F[0][:, EL_IDX].T), setup=lambda torch, inp: _i32(torch, EL_IDX)),
        _pack_case(False), _pack_case(True),
        _el_case("transform_poly", "power 3", lambda ctx, F, out, s, p: (e().transform_poly(F[0], KELVIN, 3, stream=s), None),
                 lambda inp, F: E.poly_chain(F[0], KELVIN, 3)),
        _el_case("transform_edd", "two terms", lambda ctx, F, out, s, p: (e().transform_edd(F[0], F[1], KELVIN, [(c, t) for c, t in p["terms"]], stream=s), None),
                 _edd_terms_ref, exact=False, hi=True, tol=_edd_terms_tol, skip_inf=True, params=lambda: {"terms": np.array(EDD_TERMS)}),
        _el_case("combine_planes", "three planes",
                 lambda ctx, F, out, s, p: (e().combine_planes(__import__("torch").stack([F[0], F[1], F[0] * 0.5]), p["coefs"], stream=s), None),
                 _combine_ref, exact=False, hi=True, tol=_combine_tol, params=lambda: {"coefs": np.array(COMBINE)}),
        _el_case("relayout", "order (1, 0)", lambda ctx, F, out, s, p: (e().relayout(F[0], order=(1, 0), stream=s), None),
                 lambda inp, F: np.ascontiguousarray(F[0].T)),
        _el_case("relayout", "transposed view", lambda ctx, F, out, s, p: (e().relayout(F[0].t(), stream=s), None),
                 lambda inp, F: np.ascontiguousarray(F[0].T)),
        _el_case("to_float64", "order (1, 0)", lambda ctx, F, out, s, p: (e().to_float64(F[0], order=(1, 0), stream=s), None),
                 lambda inp, F: np.ascontiguousarray(F[0].T).astype(np.float64), dtypes=(F32,)),
    ]
    return cases


CASES = _build_cases()
PARAMS = [(c, dt) for c in CASES for dt in c.dtypes]
IDS = ["%s-%s" % (c.id, np.dtype(dt).name) for c, dt in PARAMS]


def case_steps(case, inp):
    return case.own_steps(inp) if hasattr(case, "own_steps") else steps(case, inp)
