"""Stream ordering of every engine call that takes ``stream=`` (run with -m gpu), probed while a DIFFERENT stream is torch's
current one -- the case the parameter exists for.  The contract, whichever stream is current:

  1  all device work of a call -- kernels, the fills of ``out`` / ``status`` / workspaces, internal relayouts, first-use uploads
     of plan tables, the reads of the inputs -- is ordered on ``stream``, or complete before the call returns;
  2  the call waits for no other stream (the calls of BLOCKING excepted, which say so);
  3  the results are bit-equal to the same call on the idle device on the default stream.

Every entry of PROBES is run first as that reference, then through two probes built on the bounded gates of
tests/stream_gate.py (``torch.cuda._sleep``, about 0.1 s, ends by itself):

  A  late input    the floating-point operands hold NaN; the side stream gets a gate and, behind it, the copy of the real
                   values; the call is made with ``stream=side`` while the DEFAULT stream is current.  Whatever the call queued on
                   another stream read the NaN.
  B  busy current  the inputs are ready; the default (current) stream gets a gate and, behind it, a NaN fill of freed blocks of
                   the sizes of the results; the call is made with ``stream=side``.  A fill or an allocation the call made on the
                   current stream lands after the kernels: a late zero-fill clears the status word (the ``inf`` cases: one counted
                   +inf, reference status 1), a block taken from the current stream's free list is poisoned behind the gate.

In both the gate must still be held when the call returns on the host (``gate_held``): a probe whose gate has ended proves
nothing, so it fails ("gate too short / call blocked") instead of passing silently.  The late or poisoned operand is always
floating-point FIELD data in valid memory -- never a row list, an index, a day-of-year or window vector or a plan table: those go
in as synchronised int32 device tensors with ``checked=True``, so a probe can only ever produce wrong values.  ``take_axis``
uploads its index itself -- a blocking copy on torch's CURRENT stream, complete when the call returns -- and therefore has no
probe B; it is the one call that may wait for the current stream.

Shapes are the suite's smallest: the row lists of tests/test_gpu_spell.py (T = 23; 9, 8 and 0 entries) at n = 257 on the aligned
pitch and on pad + 1; ``_Sparse(16, 32)`` of tests/test_gpu_packed_totals.py; the 127 x 15 table of
tests/test_gpu_dense_forms_small.py.  tests/spell_ref.py, tests/rolling_ref.py and tests/quantile_ref.py anchor the default-stream
reference itself once each.  ``quantile_select`` is called with an explicit ``max_rows`` (the longest list, 9): ``max_rows=None`` on
device lists blocks on torch's current stream, which its docstring says.  tests/test_stream_order_host.py checks, without a GPU, that PROBES and EXEMPT cover every ``stream=`` entry point."""
import numpy as np
import pytest

from tests import stream_gate as gate
from tests.quantile_ref import quantile_ref
from tests.rolling_ref import rolling_ref
from tests.spell_ref import spell_ref
from tests.test_gpu_dense_forms_small import EDD_THRESHOLDS, OFFSET, build_plan, edd_fields, kelvin_field
from tests.test_gpu_packed_totals import _Sparse, segment_plans  # noqa: F401
from tests.test_gpu_spell import OPEN, RB, ROWS, T, _field, _pads

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
N = 257
DENSE = (127, 15)                                                # the smallest table of tests/test_gpu_dense_forms_small.py
DENSE_T = 65

# Calls that synchronise by design; each with the sentence of its docstring that says so.  Results only, no gate_held.
BLOCKING = {
    "SparsePlan.status": "Synchronise the stream and raise if any apply on this plan failed on the device",
    "ManyPlan.status": "Synchronise the stream and raise if an apply on this plan failed on the device",
    "DensePlan.saw_inf": "synchronises the stream and clears the note",
    "any_less": "blocks",
    "row lists given as host integers": "otherwise the library checks them on the device first, which blocks",
}

# Entry points with ``stream=`` that have no probe, or not both (one line each: why).
EXEMPT = {
    "profile_event_overhead": "times empty kernels on a stream and returns no data",
    "take_axis": "probe B only: it uploads its index itself, a blocking copy on the CURRENT stream (the safety rule); probe A runs",
}


class Case:
    """One call: ``fields`` (device tensors, the floating-point operands), ``call(F, stream, plan)`` -> tensors / values;
    ``make``: builds the plan handed to ``call`` anew for the reference and for every probe (a FIRST use), else None;
    ``check(ref)``: asserts on the default-stream reference (host arrays)."""

    def __init__(self, label, fields, call, probes="AB", blocking=False, make=None, check=None):
        self.label, self.fields, self.call, self.probes, self.blocking, self.make, self.check = label, fields, call, probes, blocking, make, check


def _flat(res):
    if isinstance(res, (list, tuple)):
        return [x for r in res for x in _flat(r)]
    return [res]


def _host(res):
    """the results as host arrays (tensors copied, values wrapped)"""
    return [r.cpu().numpy() if hasattr(r, "cpu") else np.asarray(r) for r in _flat(res)]


def _same_bits(got, ref, what):
    """one message per result that differs from the reference in any bit -- every result is compared, so that a poisoned ``out``
    does not hide what became of the status word beside it"""
    assert len(got) == len(ref), what
    failures = []
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and g.dtype == r.dtype, (what, i, g.shape, r.shape, g.dtype, r.dtype)
        bits = {1: np.uint8, 4: np.uint32, 8: np.uint64}[g.itemsize]
        gb, rb = np.ascontiguousarray(g).reshape(-1).view(bits), np.ascontiguousarray(r).reshape(-1).view(bits)
        if not np.array_equal(gb, rb):
            bad = np.flatnonzero(gb != rb)
            k = int(bad[0])
            failures.append("%s: result %d (%s%s) differs from the default-stream reference in %d of %d elements, first at flat index %d: "
                            "got %r, reference %r (NaN got / reference: %d / %d)" % (
                                what, i, g.dtype, list(g.shape), len(bad), g.size, k, g.reshape(-1)[k], r.reshape(-1)[k],
                                int(np.isnan(g).sum()) if g.dtype.kind == "f" else 0, int(np.isnan(r).sum()) if r.dtype.kind == "f" else 0))
    return failures


def _poison_sizes(res):
    """The sizes of the ALLOCATIONS behind the device results, each storage once -- the views a call returns (ManyPlan.apply:
    slices of one concatenated result) stand for the block they lie in, which is what ``torch.empty`` inside the call asked the
    allocator for.  A block of under 1 KiB is left alone: the status word's own late zero-fill is what its probe is after."""
    blocks = {}
    for r in _flat(res):
        if hasattr(r, "untyped_storage"):
            st = r.untyped_storage()
            blocks[st.data_ptr()] = int(st.nbytes())
    return sorted({nb for nb in blocks.values() if nb >= 1024})


def _run(torch, side, name, case):
    """reference, then the probes of ``case``; prints the gate's length and the call's host time per probe and returns the
    failures (one message per failed probe: the caller goes on with the other cases and reports them all)"""
    assert torch.cuda.current_stream() == torch.cuda.default_stream(), "the probes need the default stream current"
    what = "%s [%s]" % (name, case.label)
    blocking = case.blocking or name in BLOCKING
    torch.cuda.synchronize()
    plan = case.make() if case.make else None
    res = case.call(case.fields, None, plan)
    torch.cuda.synchronize()
    sizes = _poison_sizes(res)
    ref = _host(res)
    del res
    if plan is not None:
        plan.close()
    if case.check:
        case.check(ref)
    failures = []
    for probe in case.probes:
        plan = case.make() if case.make else None
        if probe == "A":
            twins = [_nan_twin(torch, t) for t in case.fields]
            for nb in sizes:
                gate.poisoned_block(nb)
                gate.poisoned_block(nb, side)
            torch.cuda.synchronize()
            ev = gate.blocker(side)
            with torch.cuda.stream(side):
                for tw, t in zip(twins, case.fields):
                    tw.copy_(t)
            operands = twins
        else:
            operands = case.fields
            torch.cuda.synchronize()
            ev = gate.blocker(torch.cuda.current_stream())
            for nb in sizes:
                gate.poisoned_block(nb)                         # (the fill is queued behind the gate)
        with gate.timed("%s probe %s" % (what, probe)) as tm:
            res = case.call(operands, side, plan)
        held = gate.gate_held(ev)
        side.synchronize()
        torch.cuda.synchronize()
        got = _host(res)
        if plan is not None:
            plan.close()
        print("%s probe %s: gate %.1f ms, call %.3f ms on the host, gate held at return: %s%s" % (
            what, probe, gate.gate_ms(ev), tm.ms, held, " (blocking by design)" if blocking else ""))
        failures += _same_bits(got, ref, "%s probe %s" % (what, probe))
        if not (held or blocking):
            failures.append("%s probe %s: gate too short / call blocked (gate %.1f ms, call %.3f ms)" % (what, probe, gate.gate_ms(ev), tm.ms))
    return failures


# ---- operands -------------------------------------------------------------------------------------------------------------------
def _nan_twin(torch, t):
    """a tensor of ``t``'s shape, strides and offset in a buffer of its own that is NaN throughout (a view: its whole base)"""
    base = t._base if t._base is not None else t
    return torch.full_like(base, float("nan")).as_strided(tuple(t.shape), tuple(t.stride()), t.storage_offset())


def _tdt(torch, dtype):
    return torch.float32 if dtype == F32 else torch.float64


def _dev(torch, host, pad=0):
    """a synchronised device tensor with row stride n + pad"""
    host = np.array(host, order="C")                             # (a copy: the cached fields are read-only)
    if not pad:
        return torch.from_numpy(host).cuda()
    buf = torch.zeros((host.shape[0], host.shape[1] + pad), dtype=torch.from_numpy(host[:1]).dtype, device="cuda")
    buf[:, :host.shape[1]] = torch.from_numpy(host).cuda()
    return buf[:, :host.shape[1]]


def _i32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _fields(dtype, inf=False):
    """(tasmin, tasmax) on the row lists of tests/test_gpu_spell.py: its field (values 0 .. 10), a NaN in a listed row and, with
    ``inf``, one +inf in a listed row that is in season for its cell"""
    lo = _field(N, dtype, seed=11).copy()
    hi = (lo + np.random.default_rng(12).uniform(0.0, 5.0, lo.shape)).astype(dtype)
    lo[6, 50] = np.nan
    hi[12, 77] = np.nan
    if inf:
        lo[11, 3] = hi[11, 3] = np.inf
    return lo, hi


DOY = np.arange(100, 100 + T)
WIN = np.where(np.arange(N) % 3 == 0, OPEN, 101 | 112 << 10).astype(np.int32)      # cell 3: open all year; rows 1 .. 12 elsewhere
THR = [5.0, 2.0, 8.75]
EDGES = [-np.inf, 2.0, 5.0, 8.0, np.inf]
QLEV = [0.5, 0.0, 1.0, 0.05, 0.95, 1.0 / 3.0]

# the row-list calls: name -> (two fields?, call(engine, X, X2, rb, rows, season kwargs, stream))
ROWLIST = {
    "period_reduce": (False, lambda e, X, X2, rb, rw, kw, s: e.period_reduce(X, rb, rw, poly=(-3.0, 1, 3), checked=True, stream=s)),
    "season_reduce": (True, lambda e, X, X2, rb, rw, kw, s: e.season_reduce(X, rb, rw, kw["doy"], kw["windows"], X2=X2, edd=(0.0, [2.0, 5.0]),
                                                                          checked=True, stream=s)),
    "edd_ladder_reduce": (True, lambda e, X, X2, rb, rw, kw, s: e.edd_ladder_reduce(X, X2, rb, rw, 0.0, [1.0, 2.0, 4.0, 5.0, 7.5], checked=True, stream=s, **kw)),
    "exposure_reduce": (True, lambda e, X, X2, rb, rw, kw, s: e.exposure_reduce(X, X2, rb, rw, 0.0, EDGES, checked=True, stream=s, **kw)),
    "bin_days_reduce": (False, lambda e, X, X2, rb, rw, kw, s: e.bin_days_reduce(X, rb, rw, 0.0, EDGES, checked=True, stream=s, **kw)),
    "hinge_reduce": (False, lambda e, X, X2, rb, rw, kw, s: e.hinge_reduce(X, rb, rw, 0.0, [2.0, 5.0, 8.0], power=2, checked=True, stream=s, **kw)),
    "spell_reduce": (False, lambda e, X, X2, rb, rw, kw, s: e.spell_reduce(X, rb, rw, 0.0, THR, min_length=2, stat="days", checked=True, stream=s, **kw)),
    "rolling_reduce": (False, lambda e, X, X2, rb, rw, kw, s: e.rolling_reduce(X, rb, rw, 0.0, [1, 3], stat="max", of="mean", checked=True, stream=s, **kw)),
    "quantile_select": (False, lambda e, X, X2, rb, rw, kw, s: e.quantile_select(X, rb, rw, 0.0, QLEV, max_rows=9, checked=True, stream=s, **kw)),
}
ALWAYS_SEASON = ("season_reduce",)
NEVER_SEASON = ("period_reduce",)


def _rowlist_cases(name):
    def build(torch, dtype):
        from climate_toolbox_amd import engine
        two, fn = ROWLIST[name]
        rb, rw = engine.period_lists(RB, ROWS, T)
        doy, win = _i32(torch, DOY), _i32(torch, WIN)
        seasons = [s for s in (False, True) if not (s and name in NEVER_SEASON) and not (not s and name in ALWAYS_SEASON)]
        cases = []

        def add(label, lo, hi, pad, season, lists, **kw):
            F = [_dev(torch, lo, pad)] + ([_dev(torch, hi, pad)] if two else [])
            skw = dict(doy=doy, windows=win) if season else {}
            cases.append(Case(label, F, lambda F, s, plan: fn(engine, F[0], F[1] if two else None, lists[0], lists[1], skw, s), **kw))

        lo, hi = _fields(dtype)
        for pad in _pads(N, dtype):
            for season in seasons:
                check = None
                if name == "spell_reduce" and season and pad == _pads(N, dtype)[0]:
                    def check(ref):
                        assert np.array_equal(ref[0].astype(np.float64), spell_ref(lo, RB, ROWS, 0.0, THR, 2, "days", "above", DOY, WIN)) and ref[1].tolist() == [0]
                if name == "rolling_reduce" and season and pad == _pads(N, dtype)[0]:
                    def check(ref):
                        assert np.array_equal(ref[0], rolling_ref(lo, RB, ROWS, 0.0, [1, 3], "max", "mean", DOY, WIN), equal_nan=True) and ref[1].tolist() == [0]
                if name == "quantile_select" and season and pad == _pads(N, dtype)[0]:
                    def check(ref):
                        assert np.array_equal(ref[0], quantile_ref(lo, RB, ROWS, 0.0, QLEV, "linear", DOY, WIN), equal_nan=True) and ref[1].tolist() == [0]
                add("pad %d, %s" % (pad, "season" if season else "no season"), lo, hi, pad, season, (rb, rw), check=check)
        # the status word: one counted +inf, so the reference reads 1 -- a zero-fill that lands late reads 0
        ilo, ihi = _fields(dtype, inf=True)

        def is_one(ref):
            assert ref[1].tolist() == [1], "the reference status must be 1 for the probe to mean anything, got %r" % (ref[1],)
        add("inf: status word", ilo, ihi, 0, seasons[-1], (rb, rw), check=is_one)
        # host lists: checked and uploaded by the call, which therefore blocks (BLOCKING): results only
        add("host lists", lo, hi, 0, seasons[-1], (RB, ROWS), blocking=True)
        return cases
    return build


def _season_mask(torch, dtype):
    from climate_toolbox_amd import engine
    doy, win = _i32(torch, DOY), _i32(torch, WIN)
    return [Case("device vectors", [], lambda F, s, plan: engine.season_mask(doy, win, stream=s))]


def _gather(torch, dtype):
    from climate_toolbox_amd import engine
    lo, _ = _fields(dtype)
    idx = _i32(torch, np.random.default_rng(2).integers(0, N, 100))
    return [Case("TG -> TR", [_dev(torch, lo)], lambda F, s, plan: engine.gather(F[0], idx, stream=s)),
            Case("TG -> RT, pitched", [_dev(torch, lo, 3)], lambda F, s, plan: engine.gather(F[0], idx, out_layout="RT", stream=s))]


def _transform_poly(torch, dtype):
    from climate_toolbox_amd import engine
    lo, _ = _fields(dtype)
    return [Case("contiguous", [_dev(torch, lo)], lambda F, s, plan: engine.transform_poly(F[0], -3.0, 3, stream=s)),
            Case("transposed view", [_dev(torch, lo.T).t()], lambda F, s, plan: engine.transform_poly(F[0], -3.0, 3, stream=s))]


def _transform_edd(torch, dtype):
    from climate_toolbox_amd import engine
    lo, hi = _fields(dtype)
    terms = [(1.0, 2.0), (-1.0, 8.0)]
    return [Case("contiguous", [_dev(torch, lo), _dev(torch, hi)], lambda F, s, plan: engine.transform_edd(F[0], F[1], 0.0, terms, stream=s)),
            Case("transposed views", [_dev(torch, lo.T).t(), _dev(torch, hi.T).t()], lambda F, s, plan: engine.transform_edd(F[0], F[1], 0.0, terms, stream=s))]


def _combine_planes(torch, dtype):
    from climate_toolbox_amd import engine
    lo, hi = _fields(dtype)
    return [Case("three planes", [_dev(torch, np.stack([lo, hi, lo * dtype(0.5)]))], lambda F, s, plan: engine.combine_planes(F[0], [1.0, -2.0, 0.25], stream=s))]


def _relayout(torch, dtype):
    from climate_toolbox_amd import engine
    lo, _ = _fields(dtype)
    return [Case("transposed view", [_dev(torch, lo.T).t()], lambda F, s, plan: engine.relayout(F[0], stream=s)),
            Case("order (1, 0), pitched", [_dev(torch, lo, 3)], lambda F, s, plan: engine.relayout(F[0], order=(1, 0), stream=s))]


def _to_float64(torch, dtype):
    from climate_toolbox_amd import engine
    lo, _ = _fields(dtype)
    return [Case("transposed view", [_dev(torch, lo.T).t()], lambda F, s, plan: engine.to_float64(F[0], stream=s)),
            Case("order (1, 0)", [_dev(torch, lo)], lambda F, s, plan: engine.to_float64(F[0], order=(1, 0), stream=s))]


def _take_axis(torch, dtype):
    from climate_toolbox_amd import engine
    lo, _ = _fields(dtype)
    index = np.random.default_rng(4).permutation(N)[:200]
    return [Case("contiguous", [_dev(torch, lo)], lambda F, s, plan: engine.take_axis(F[0], 1, index, stream=s), probes="A"),
            Case("transposed view", [_dev(torch, lo.T).t()], lambda F, s, plan: engine.take_axis(F[0], 1, index, stream=s), probes="A")]


def _any_less(torch, dtype):
    from climate_toolbox_amd import engine
    lo, hi = _fields(dtype)
    lo, hi = np.nan_to_num(lo, nan=1.0), np.nan_to_num(hi, nan=9.0)
    hi2 = hi.copy()
    hi2[20, 200] = lo[20, 200] - dtype(1.0)                       # the one element that is less

    def true(ref):
        assert ref[0].tolist() is True

    def false(ref):
        assert ref[0].tolist() is False
    return [Case("one less", [_dev(torch, hi2), _dev(torch, lo)], lambda F, s, plan: engine.any_less(F[0], F[1], stream=s), check=true),
            Case("one less, transposed views", [_dev(torch, hi2.T).t(), _dev(torch, lo.T).t()], lambda F, s, plan: engine.any_less(F[0], F[1], stream=s), check=true),
            Case("none less", [_dev(torch, hi), _dev(torch, lo)], lambda F, s, plan: engine.any_less(F[0], F[1], stream=s), check=false)]


# ---- plans ----------------------------------------------------------------------------------------------------------------------
def _sparse(dtype):
    return _Sparse(16, 32, dtype, seed=5)


def _celsius(c, torch):
    tas = c.tas.reshape(c.T, c.G)
    return _dev(torch, tas), _dev(torch, c.tasmax.reshape(c.T, c.G))


def _first_and_later(label, fields, call, c, keep, **kw):
    """``call`` on a plan that has applied before (the reference's) and on one that has not (made anew for every run)"""
    plan = c.plan()
    keep.append(plan)
    return [Case(label + ", later use", fields, lambda F, s, _: call(plan, F, s), **kw),
            Case(label + ", first use", fields, lambda F, s, fresh: call(fresh, F, s), probes="A", make=c.plan, **kw)]


def _sparse_apply(torch, dtype, keep):
    from climate_toolbox_amd import engine
    c = _sparse(dtype)
    tas, _ = _celsius(c, torch)
    packer = c.plan()
    keep.append(packer)
    packed = engine.pack_rows(packer, tas)
    torch.cuda.synchronize()
    return (_first_and_later("plain", [tas], lambda p, F, s: p.apply(F[0], stream=s), c, keep) +
            _first_and_later("RT", [tas], lambda p, F, s: p.apply(F[0], out_layout="RT", stream=s), c, keep) +
            _first_and_later("compact rows", [packed], lambda p, F, s: p.apply(F[0], compact=True, stream=s), c, keep))


def _sparse_apply_poly(torch, dtype, keep):
    c = _sparse(dtype)
    tas, _ = _celsius(c, torch)
    return _first_and_later("three powers", [tas], lambda p, F, s: p.apply_poly(F[0], -273.15, 3, stream=s), c, keep)


def _sparse_apply_edd(torch, dtype, keep):
    c = _sparse(dtype)
    tas, tasmax = _celsius(c, torch)
    return _first_and_later("two thresholds", [tas, tasmax], lambda p, F, s: p.apply_edd(F[0], F[1], [285.0, 290.0], stream=s), c, keep)


def _sparse_status(torch, dtype, keep):
    c = _sparse(dtype)
    tas, _ = _celsius(c, torch)

    def call(p, F, s):
        out = p.apply(F[0], stream=s)
        p.status(stream=s)
        return out
    return _first_and_later("apply, then status", [tas], call, c, keep)


def _pack_rows(torch, dtype, keep):
    from climate_toolbox_amd import engine
    c = _sparse(dtype)
    tas, tasmax = _celsius(c, torch)
    plan = c.plan()
    keep.append(plan)
    return [Case("one field", [tas], lambda F, s, _: engine.pack_rows(plan, F[0], stream=s)),
            Case("two fields", [tas, tasmax], lambda F, s, _: engine.pack_rows(plan, F[0], F[1], stream=s))]


def _many(c):
    from climate_toolbox_amd import engine
    return engine.ManyPlan(c.cell, c.code, [c.w_eff, c.df["areawt"].to_numpy()], c.G, c.R, row_len=c.nlon,
                           levels=[(c.code // 4, (c.R + 3) // 4)])


def _many_apply(torch, dtype, keep):
    c = _sparse(dtype)
    tas, _ = _celsius(c, torch)
    plan = _many(c)
    keep.append(plan)
    return [Case("two weightings, two levels, later use", [tas], lambda F, s, _: plan.apply(F[0], stream=s)),
            Case("two weightings, two levels, first use", [tas], lambda F, s, fresh: fresh.apply(F[0], stream=s), probes="A", make=lambda: _many(c))]


def _many_status(torch, dtype, keep):
    c = _sparse(dtype)
    tas, _ = _celsius(c, torch)
    plan = _many(c)
    keep.append(plan)

    def call(F, s, _):
        out = plan.apply(F[0], stream=s)
        plan.status(stream=s)
        return out
    return [Case("apply, then status", [tas], call)]


def _dense_forms(dtype):
    """(label, form, exact) of the dense-family forms that serve ``dtype``"""
    if dtype == F32:
        return [("full, split", "full", False), ("full, exact", "full", True), ("tiles", "tiles", False), ("entries", "entries", False)]
    return [("full", "full", False), ("tiles", "tiles", False), ("entries", "entries", False)]


def _dense(kind):
    def build(torch, dtype, keep):
        G, R = DENSE
        X = _dev(torch, kelvin_field(G, R, dtype, DENSE_T))
        lo, hi = (_dev(torch, f) for f in edd_fields(G, R, dtype, DENSE_T))
        cases = []
        for label, form, exact in _dense_forms(dtype):
            plan = build_plan(G, R, form, dtype)
            keep.append(plan)
            if kind == "apply":
                cases.append(Case(label, [X], lambda F, s, _, plan=plan, exact=exact: plan.apply(F[0], stream=s, exact=exact)))
            elif kind == "poly":
                cases.append(Case(label, [X], lambda F, s, _, plan=plan, exact=exact: plan.apply_poly(F[0], OFFSET, 2, stream=s, exact=exact)))
            elif kind == "edd":
                cases.append(Case(label, [lo, hi], lambda F, s, _, plan=plan, exact=exact: plan.apply_edd(F[0], F[1], EDD_THRESHOLDS[1], stream=s, exact=exact)))
            else:
                Xi = kelvin_field(G, R, dtype, DENSE_T).copy()
                Xi[3, 0] = np.inf                                # cell 0 holds a pair in every table

                def call(F, s, _, plan=plan, exact=exact):
                    out = plan.apply(F[0], stream=s, exact=exact)
                    return out, plan.saw_inf(stream=s)
                cases.append(Case(label + ", +inf", [_dev(torch, Xi)], call))
        return cases
    return build


def _no_plans(build):
    return lambda torch, dtype, keep: build(torch, dtype)


# name of the entry point (as tests/test_stream_order_host.py collects them) -> (element types, builder of its cases)
BOTH = (F32, F64)
PROBES = {name: (BOTH, _no_plans(_rowlist_cases(name))) for name in ROWLIST}
PROBES.update({
    "season_mask": ((F64,), _no_plans(_season_mask)),
    "gather": (BOTH, _no_plans(_gather)),
    "pack_rows": (BOTH, _pack_rows),
    "transform_poly": (BOTH, _no_plans(_transform_poly)),
    "transform_edd": (BOTH, _no_plans(_transform_edd)),
    "combine_planes": (BOTH, _no_plans(_combine_planes)),
    "relayout": (BOTH, _no_plans(_relayout)),
    "to_float64": (BOTH, _no_plans(_to_float64)),
    "take_axis": (BOTH, _no_plans(_take_axis)),
    "any_less": (BOTH, _no_plans(_any_less)),
    "SparsePlan.apply": (BOTH, _sparse_apply),
    "SparsePlan.apply_poly": (BOTH, _sparse_apply_poly),
    "SparsePlan.apply_edd": (BOTH, _sparse_apply_edd),
    "SparsePlan.status": (BOTH, _sparse_status),
    "ManyPlan.apply": (BOTH, _many_apply),
    "ManyPlan.status": (BOTH, _many_status),
    "DensePlan.apply": (BOTH, _dense("apply")),
    "DensePlan.apply_poly": (BOTH, _dense("poly")),
    "DensePlan.apply_edd": (BOTH, _dense("edd")),
    "DensePlan.saw_inf": (BOTH, _dense("saw_inf")),
})
PARAMS = [(name, dtype) for name, (dtypes, _) in PROBES.items() for dtype in dtypes]


@pytest.fixture(scope="module")
def streams():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    gate.calibrate(torch)
    first = len(gate.NOTES)
    yield torch, torch.cuda.Stream()
    # the report of this module's probes, whichever of them ran: the gate's target and the largest host times
    calls = [(w, t) for w, t in gate.NOTES[first:] if " probe " in w]
    print("\ngate: target %.0f ms; %d probed calls" % (gate.GATE_MS, len(calls)))
    if calls:
        print("largest host time of a probed call: %.3f ms (%s)" % max(((t, w) for w, t in calls)))
        quick = [(t, w) for w, t in calls if "host lists" not in w and not any(w.startswith(b + " ") for b in BLOCKING)]
        if quick:
            print("largest host time of a probed call that is not blocking by design: %.3f ms (%s)" % max(quick))


@pytest.mark.parametrize("name,dtype", PARAMS, ids=["%s-%s" % (n, np.dtype(d).name) for n, d in PARAMS])
def test_stream_order(streams, segment_plans, name, dtype):
    """Every case of PROBES[name]: the default-stream reference, probe A (late input) and probe B (busy current stream), results
    bit-equal and the gate still held when the call returns (the module's docstring has the protocol)."""
    torch, side = streams
    keep, failures = [], []
    try:
        for case in PROBES[name][1](torch, dtype, keep):
            failures += _run(torch, side, name, case)
    finally:
        torch.cuda.synchronize()
        for plan in keep:
            plan.close()
    assert not failures, "%d probe(s) failed:\n%s" % (len(failures), "\n".join(failures))


def test_a_gate_lasts_what_it_was_calibrated_to(streams):
    """A gate is held right after it is queued and lasts about GATE_MS by its own events (within a factor of four either way:
    the probes need tens of milliseconds, not an exact length)."""
    torch, side = streams
    ev = gate.blocker(side)
    held = gate.gate_held(ev)
    ms = gate.gate_ms(ev)
    print("gate: target %.0f ms, measured %.1f ms" % (gate.GATE_MS, ms))
    assert held and 0.25 * gate.GATE_MS <= ms <= 4.0 * gate.GATE_MS, "the gate does not last what it was calibrated to: %.1f ms" % ms
