"""relative.cell_spell_reduce(plane_of_row=) on streams and in a captured graph (run with -m gpu): the stream-order probes of
tests/test_gpu_cell_spell_streams.py for wagg_row_cell_spells_*, by the protocol and with the helpers of
tests/test_gpu_stream_order.py (tests/stream_gate.py's bounded gates), and one capture-and-replay case after
tests/test_gpu_graph_replay.py's pattern.

Stream order: probe A hands the call NaN twins of the field AND of the thresholds whose real values arrive on the side stream
behind a gate; probe B holds the current stream busy while the call runs on the side stream.  Graph: ``checked=True``, device
lists, a device row map, a season -- the non-blocking path; captured once on a side stream, replayed after the field and the
thresholds were overwritten in place; every replay equals the NumPy restatement exactly."""
import numpy as np
import pytest

from tests.cell_spell_rows_ref import cell_spell_rows_ref
from tests.test_gpu_spell import OPEN, RB, ROWS, T, _field, _pads
from tests.test_gpu_stream_order import Case, _dev, _i32, _run
from tests import stream_gate as gate

pytestmark = pytest.mark.gpu

N = 257
M = 3
DOY = np.arange(100, 100 + T)
WIN = np.where(np.arange(N) % 3 == 0, OPEN, 101 | 112 << 10).astype(np.int32)
PMAP = ((np.arange(T) * 5 + 1) % M).astype(np.int32)


def _operands(dtype, inf=False):
    X = _field(N, dtype, seed=11).copy()
    X[6, 50] = np.nan
    if inf:
        X[11, 3] = np.inf                                                                 # (cell 3 is open all year)
    thr = np.random.default_rng(21).uniform(1.0, 9.5, (5, M, N)).astype(dtype)
    thr[2, 1, 9] = np.nan
    return X, thr


@pytest.fixture(scope="module")
def streams():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    gate.calibrate(torch)
    yield torch, torch.cuda.Stream()
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_stream_order(streams, dtype):
    """Counts under a season and the fp64 excess without one, aligned and unaligned rows; the status word with one counted +inf."""
    from climate_toolbox_amd import engine
    from climate_toolbox_amd.relative import cell_spell_reduce
    torch, side = streams
    rb, rw = engine.period_lists(RB, ROWS, T)
    doy, win, pmap = _i32(torch, DOY), _i32(torch, WIN), _i32(torch, PMAP)
    X, thr = _operands(dtype)
    cases = []

    def add(label, Xh, pad, kw, season, check=None):
        skw = dict(doy=doy, windows=win) if season else {}
        F = [_dev(torch, Xh, pad), _dev(torch, thr.reshape(5 * M, N), pad)]
        call = lambda F, s, plan: cell_spell_reduce(F[0], rb, rw, 0.0, F[1].unflatten(0, (5, M)), checked=True, stream=s, plane_of_row=pmap,
                                                    **kw, **skw)
        cases.append(Case(label, F, call, check=check))

    for pad in _pads(N, dtype):
        def check(ref, pad=pad):
            want = cell_spell_rows_ref(X, RB, ROWS, 0.0, thr, PMAP, 2, "days", "above", DOY, WIN).astype(dtype)
            assert np.array_equal(ref[0], want, equal_nan=True) and ref[1].tolist() == [0]
        add("pad %d, days, season" % pad, X, pad, dict(min_length=2, stat="days"), True, check)
        add("pad %d, excess below, no season" % pad, X, pad, dict(stat="excess", side="below"), False)
    Xi, _ = _operands(dtype, inf=True)

    def is_one(ref):
        assert ref[1].tolist() == [1], "the reference status must be 1 for the probe to mean anything, got %r" % (ref[1],)
    add("inf: status word", Xi, 0, dict(min_length=2, stat="events"), True, is_one)
    failures = []
    for case in cases:
        failures += _run(torch, side, "cell_spell_reduce(plane_of_row=)", case)
    torch.cuda.synchronize()
    assert not failures, "%d probe(s) failed:\n%s" % (len(failures), "\n".join(failures))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_graph_capture_and_replay(streams, dtype):
    """Captured once; replayed over a halved field, fresh thresholds, a NaN threshold plane and a counted +inf: every replay writes
    the whole result, equals the restatement bit for bit, and the status word is set on the +inf step alone."""
    from climate_toolbox_amd import engine
    from climate_toolbox_amd.relative import cell_spell_reduce
    torch, side = streams
    n = 1029
    pad = _pads(n, dtype)[0]
    X0 = _field(n, dtype, seed=5)
    thr0 = np.random.default_rng(6).uniform(1.0, 9.5, (5, M, n)).astype(dtype)
    win_h = np.where(np.arange(n) % 3 == 0, OPEN, 101 | 112 << 10).astype(np.int32)
    rb, rw = engine.period_lists(RB, ROWS, T)
    doy, win, pmap = _i32(torch, DOY), _i32(torch, win_h), _i32(torch, PMAP)
    Xd = _dev(torch, X0, pad)
    thr_d = _dev(torch, thr0.reshape(5 * M, n), pad).unflatten(0, (5, M))
    out = torch.empty((5, 3, n), dtype=Xd.dtype, device="cuda")
    kw = dict(min_length=2, stat="days", side="above", doy=doy, windows=win, checked=True, plane_of_row=pmap)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        cell_spell_reduce(Xd, rb, rw, 0.0, thr_d, stream=side, **kw)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    try:
        with torch.cuda.graph(g, stream=side):
            res, status = cell_spell_reduce(Xd, rb, rw, 0.0, thr_d, out=out, stream=side, **kw)
        assert res is out
        half = (X0 * dtype(0.5)).astype(dtype)
        thr1 = np.random.default_rng(7).uniform(0.5, 5.0, (5, M, n)).astype(dtype)
        thr2 = thr1.copy()
        thr2[3, 1] = np.nan
        Xinf = half.copy()
        Xinf[6, 0] = np.inf                                                               # cell 0: open all year, row 6 is listed
        for label, Xh, th in (("half", half, thr0), ("fresh thresholds", half, thr1), ("NaN thresholds", X0, thr2),
                              ("inf", Xinf, thr1), ("clean", X0, thr0)):
            Xd.copy_(torch.from_numpy(Xh))
            thr_d.copy_(torch.from_numpy(th))
            out.fill_(float("nan"))
            status.fill_(0x5A5A5A)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            want = cell_spell_rows_ref(Xh, RB, ROWS, 0.0, th, PMAP, 2, "days", "above", DOY, win_h).astype(dtype)
            assert np.array_equal(out.cpu().numpy(), want, equal_nan=True), label
            assert int(status.item()) == (1 if label == "inf" else 0), (label, int(status.item()))
            eager, st = cell_spell_reduce(Xd, rb, rw, 0.0, thr_d, **kw)
            assert np.array_equal(eager.cpu().numpy(), out.cpu().numpy(), equal_nan=True) and int(st.item()) == int(status.item()), label
    finally:
        torch.cuda.synchronize()
        del g
