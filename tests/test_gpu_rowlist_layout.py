"""The eighteen row-list entry points (wagg_{period,season,edd_ladder,bin_days,hinge,exposure,spell,rolling}_reduce_f32 / _f64
and wagg_quantile_select_f32 / _f64) called through ctypes with what the binding never hands them (run with -m gpu; tests/rowlist_layout.py has the layouts and the
case table): a pitched result (ldo = n + 5, out_pstride = P * ldo + 7) at a 16-byte boundary and one element past it, fields
that are views into poisoned buffers, field bases one element off a 16-byte boundary (both fields, and tasmax alone), and
workspaces of the family's own size, of three parts, of one part and none.  The period quantiles have no *_work_bytes and
promise to ignore the argument: they get the same four workspaces ("full" being three parts) and must leave every byte of them.

Every call is checked four ways: against the family's reference on the unpoisoned logical field (exact where the family's own
test is exact, else RTOL32 / RTOL64 with that test's scale); bit for bit against the binding's call on a zero-padded view of
the same pitch and base alignment (with a cut-down workspace only the families whose bits do not depend on the split); the
status word is 0 although NaN, +-inf and 1e30 stand in every pad, unlisted row, out-of-season day and guard; and nothing but
out[k][p][0:n] and the first work_bytes of the workspace has changed, bit for bit.  One control per family puts a +inf into a
listed, in-season cell: bit 0 comes up, so the zeros mean something.

Which route a call took is not visible in its numbers -- a 16-byte load from a base that is one element off returns the right
cells on this hardware -- so one more shape makes it visible in the workspace: n = 4097 with 512 entries in one period is cut
into 64 parts in 16-byte pieces and into 61 at one cell per lane (test_the_route_decides_the_parts)."""
import numpy as np
import pytest

from tests import rowlist_layout as RL

pytestmark = pytest.mark.gpu

DT_IDS = {RL.F32: "f32", RL.F64: "f64"}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _bits_dtype(torch, t):
    return torch.int32 if t.element_size() == 4 else torch.int64


def _sentinel_filled(torch, numel, tdtype):
    t = torch.empty(numel, dtype=tdtype, device="cuda")
    t.view(_bits_dtype(torch, t)).fill_(RL.SENTINEL[t.element_size()])
    return t


def _view(torch, flat, start, T, ldx, n, shift):
    dev = torch.from_numpy(flat).cuda()
    v = dev[start:start + T * ldx].view(T, ldx)[:, :n]
    assert v.stride(0) == ldx and v.data_ptr() % 16 == shift * dev.element_size()
    return v


class _Case:
    """the buffers of one (case, family, dtype): poisoned fields for the C-ABI calls, zero-padded twins for the binding"""

    def __init__(self, torch, fam, dtype, lists, route, n, seasoned, inf_at=None):
        from climate_toolbox_amd import engine
        self.torch, self.fam, self.route = torch, fam, route
        d = self.d = RL.make_data(lists, n, dtype, RL.seasoned_for(fam, seasoned), inf_at=inf_at)
        self.ldx = RL.ldx_for(route, n, dtype)
        sx, s2 = RL.shifts_for(route)
        self.X = _view(torch, *RL.poisoned(d.X, d.live, self.ldx, sx), d.T, self.ldx, n, sx)
        self.X2 = _view(torch, *RL.poisoned(d.H, d.live, self.ldx, s2), d.T, self.ldx, n, s2)
        self.tX = _view(torch, *RL.zero_padded(d.X, self.ldx, sx), d.T, self.ldx, n, sx)
        self.tX2 = _view(torch, *RL.zero_padded(d.H, self.ldx, s2), d.T, self.ldx, n, s2)      # (the binding asks one pitch of the two
        self.call = engine._RowlistCall(self.X, d.rb, d.rows, False, (d.doy, d.win) if d.seasoned else None)      # fields, any base)
        assert self.call.P == d.P and self.call.n_rows == len(d.rows)

    def twin(self, v):
        from climate_toolbox_amd import engine
        out, st = self.fam.twin(engine, self.tX, self.tX2, self.d, v)
        return out, int(st.item())

    def run(self, v, out_off, work_kind):
        """one C-ABI call: (the (planes, P, n) result, the status word, the parts the list was cut into)"""
        from climate_toolbox_amd import _lib, engine
        torch, fam, d, c = self.torch, self.fam, self.d, self.call
        L = _lib.load()
        lay = RL.out_layout(v.planes, d.P, d.n, out_off)
        buf = _sentinel_filled(torch, lay.total, self.X.dtype)
        es = buf.element_size()
        out_ptr = buf.data_ptr() + lay.start * es
        assert buf.data_ptr() % 16 == 0 and out_ptr % 16 == out_off * es
        full = RL.full_work_bytes(L, fam, v, d.n, d.P, len(d.rows))
        wb = RL.work_bytes_of(work_kind, full, v.planes, d.P, d.n)
        work = _sentinel_filled(torch, wb // 8 + RL.GUARD, torch.float64) if wb else None
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        args, keep = RL.build_args(fam, v, dict(
            X=self.X.data_ptr(), X2=self.X2.data_ptr(), T=d.T, n=d.n, ldx=self.ldx, rb=c.row_begin.data_ptr(), rows=c.rows.data_ptr(),
            P=c.P, n_rows=c.n_rows, doy=c.doy.data_ptr() if d.seasoned else None, win=c.windows.data_ptr() if d.seasoned else None,
            flags=c.flags, out=out_ptr, ldo=lay.ldo, pstride=lay.pstride, status=status.data_ptr(),
            work=work.data_ptr() if wb else None, work_bytes=wb, stream=engine._stream_handle(None), longest=RL.longest_list(d.rb)))
        name = RL.symbol(fam, d.dtype)
        _lib.check(getattr(L, name)(*args), name)
        torch.cuda.synchronize()
        del keep
        # memory outside the result: the ldo gaps, the pstride gaps, both guards
        bits = buf.view(_bits_dtype(torch, buf)).cpu().numpy()
        idx = RL.inside_index(lay)
        outside = np.ones(lay.total, dtype=bool)
        outside[idx.ravel()] = False
        touched = np.flatnonzero(outside & (bits != RL.SENTINEL[es]))
        assert len(touched) == 0, "%d elements outside out[k][p][0:n] changed, first at %d (out_dev + %d)" % (
            len(touched), touched[0], touched[0] - lay.start)
        assert (bits[idx] != RL.SENTINEL[es]).all(), "an element of out[k][p][0:n] was not written"
        got = bits[idx].view(d.dtype)
        # the workspace: nothing behind work_bytes; nothing at all where the list is summed in one part -- or where the family
        # has no *_work_bytes and ignores the argument (fam.splits is False for it)
        assert fam.work_bytes is not None or (not fam.splits and (work_kind == "none") == (wb == 0))
        lanes = RL.vec(d.dtype) if RL.is_wide(self.route, d.dtype, d.n, v.two_fields) else 1
        split = RL.expected_split(work_kind, full, v.planes, d.P, d.n, len(d.rows), lanes) if fam.splits else 1
        if wb:
            wbits = work.view(torch.int64).cpu().numpy()
            used = split * RL.per_part(v.planes, d.P, d.n) // 8 if split > 1 else 0
            assert used <= wb // 8
            changed = np.flatnonzero(wbits[used:] != RL.SENTINEL[8])
            assert len(changed) == 0, "the workspace changed at double %d of %d (the call may use %d)" % (used + changed[0], wb // 8, used)
            assert (wbits[:used] != RL.SENTINEL[8]).all(), "a partial sum of the %d parts was not written" % split
        return got, int(status.item()), split


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(u), b.view(u))


@pytest.mark.parametrize("dtype", RL.DTYPES, ids=[DT_IDS[d] for d in RL.DTYPES])
@pytest.mark.parametrize("family", sorted(RL.FAMILIES))
def test_pitched_offset_and_poisoned_layouts(torch_cuda, family, dtype):
    """Every case of tests/rowlist_layout.py CASES for one family and element type: the three routes (and tasmax alone off its
    boundary for the calls that read it), n = 5 / 257 / 1029, the small lists and the one split list of 70 entries, with and
    without a season, both result bases, every workspace size."""
    fam = RL.FAMILIES[family]
    ran = set()
    for (lists, route, n, seasoned, out_off), cid in zip(RL.CASES, RL.CASE_IDS):
        variants = RL.variants_for(fam, route)
        if not variants:
            continue
        case = _Case(torch_cuda, fam, dtype, lists, route, n, seasoned)
        for v in variants:
            want, wst = case.twin(v)
            want = want.cpu().numpy()
            assert wst == 0, (cid, v.id)
            for kind in RL.works_for(lists):
                what = (family, cid, v.id, kind)
                got, st, split = case.run(v, out_off, kind)
                assert st == 0, what                       # pads, unlisted rows, out-of-season days: never looked at
                fam.check(got, case.d, v)
                if kind == "full" or fam.counting:
                    assert _same_bits(got, want), what
                if lists == "split" and fam.splits:
                    assert split == {"full": RL.SPLIT_PARTS, "three": 3, "one": 1, "none": 1}[kind], what
                else:
                    assert split == 1, what
                ran.add((route, kind))
    routes = {r for r in RL.ROUTES if RL.variants_for(fam, r)}
    assert ran == {(r, k) for r in routes for k in RL.WORKS}, sorted(ran)


@pytest.mark.parametrize("dtype", RL.DTYPES, ids=[DT_IDS[d] for d in RL.DTYPES])
@pytest.mark.parametrize("family", sorted(RL.FAMILIES))
def test_a_listed_in_season_infinity_sets_the_status_word(torch_cuda, family, dtype):
    """The control of the zeros above: the same poisoned layout with ONE +inf in a listed, in-season cell (row 1 of cell 0,
    open all year) sets bit 0, on the 16-byte route and on the one-cell route; everything outside the result stays untouched."""
    fam = RL.FAMILIES[family]
    for route, n in (("1", 5), ("2", 257)):
        case = _Case(torch_cuda, fam, dtype, "small", route, n, True, inf_at=(1, 0))
        assert case.d.live[1, 0]
        for v in fam.variants:
            _, st, _ = case.run(v, 1, "full")
            assert st == 1, (family, route, v.id)


TWO_FIELD = sorted(name for name, f in RL.FAMILIES.items() if RL.variants_for(f, "3b"))


@pytest.mark.parametrize("dtype", RL.DTYPES, ids=[DT_IDS[d] for d in RL.DTYPES])
@pytest.mark.parametrize("family", TWO_FIELD)
def test_the_route_decides_the_parts(torch_cuda, family, dtype):
    """n = 4097 with one list of 512 entries: 64 parts in 16-byte pieces, 61 at one cell per lane.  With tasmin on a 16-byte
    boundary and tasmax one element past one the call must take the one-cell route: the last three of the 64 parts the
    family's *_work_bytes holds stay untouched, the first 61 are all written, and the result has the bits of the binding's call
    on fields placed the same way."""
    fam = RL.FAMILIES[family]
    for lists, route, n, seasoned, out_off in RL.LONG_CASES:
        case = _Case(torch_cuda, fam, dtype, lists, route, n, seasoned)
        for v in RL.variants_for(fam, "3b"):
            want, wst = case.twin(v)
            got, st, split = case.run(v, out_off, "full")
            assert st == 0 and wst == 0 and split == RL.LONG_PARTS[route == "1"], (family, route, v.id, split)
            fam.check(got, case.d, v)
            assert _same_bits(got, want.cpu().numpy()), (family, route, v.id)
