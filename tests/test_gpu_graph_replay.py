"""Graph capture and replay of every stream-ordered engine call that docs/STREAM_CAPTURE.md lists as capturable (run with -m gpu).
The cases, their restatements and tolerances and the mutation list are tests/graph_replay.py's; tests/test_graph_replay_host.py
shows without a GPU that every mutation changes every case's expected result.

Per case: warm up on a side stream (twice for the split dense form) and synchronise; capture the call ONCE on that stream into a
single-stream graph (``out`` handed in where the call takes one; the status word and the workspace are the call's own, so their
allocation and the zero-fill of the status word are part of the graph -- two row-list cases hand in their own status word and
no workspace instead, and reset the word themselves); overwrite and drop the host parameter arrays; then, per
mutation: write the mutated fields into the SAME device tensors, refill the result with a NaN payload no arithmetic produces, poison the
status word, replay, and require

  (a) no sentinel left in the result;
  (b) the bits of the same call made eagerly now, into other buffers;
  (c) the NumPy restatement within the case's existing tolerance (on the +inf step without the row / column that holds the +inf);
  (d) the status word / ``saw_inf`` of the eager call: set on the +inf step, clear on every other one.

Between the second and the third replay unrelated eager work runs on another stream and draws on the same pools (another
segment-table plan's apply, a row-list reduction with a workspace, transform_poly).  No plan is closed and no scratch is released
while a graph is alive."""
import numpy as np
import pytest

from tests import graph_replay as GR
from tests.rowlist_layout import SENTINEL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from climate_toolbox_amd import engine
    side, other = torch.cuda.Stream(), torch.cuda.Stream()
    # the unrelated work of step 4: a plan of its own and its operands, built once
    c = GR._sparse(np.float32, seed=9)
    plan = c.plan()
    tas = GR._dev(torch, np.array(c.tas).reshape(c.T, c.G))
    d = GR.RL.make_data("replay", 257, np.float64, False, seed=3)
    X = GR._dev(torch, d.X)
    rb, rw = engine.period_lists(d.rb, d.rows, d.T)
    torch.cuda.synchronize()

    def noise():
        with torch.cuda.stream(other):
            a = plan.apply(tas, stream=other)
            b, st = engine.period_reduce(X, rb, rw, poly=(GR.KELVIN, 1, 3), checked=True, stream=other)
            e = engine.transform_poly(tas, GR.KELVIN, 2, stream=other)
        other.synchronize()
        assert int(st.item()) == 0 and a.shape[0] == c.T and b.shape[0] == 3 and e.shape == tas.shape

    yield torch, side, noise
    torch.cuda.synchronize()
    plan.close()


def _fill_sentinel(torch, t):
    flat = t.view(torch.int32 if t.element_size() == 4 else torch.int64)
    flat.fill_(SENTINEL[t.element_size()])


def _has_sentinel(a):
    return bool((GR.bits(a) == SENTINEL[a.itemsize]).any())


def _device_fields(torch, case, inp):
    """the fields as device tensors; a row-list case at n = 1029 on its 16-byte pitch (a view of a wider buffer)"""
    F = []
    for f in inp.fields:
        pitch = case.pitch(f.shape[1], f.dtype) if hasattr(case, "pitch") else f.shape[1]
        if pitch == f.shape[1]:
            F.append(GR._dev(torch, f))
        else:
            buf = torch.zeros((f.shape[0], pitch), dtype=torch.from_numpy(np.array(f[:1])).dtype, device="cuda")
            view = buf[:, :f.shape[1]]
            view.copy_(torch.from_numpy(np.array(f)))
            F.append(view)
    return F


@pytest.mark.parametrize("case,dtype", GR.PARAMS, ids=GR.IDS)
def test_graph_replay(gpu, case, dtype):
    torch, side, noise = gpu
    inp = case.build(dtype)
    ctx = case.setup(torch, inp)
    saw = ctx.saw_inf if case.status == "saw_inf" else None
    g = None
    try:
        F = _device_fields(torch, case, inp)
        fresh_params = lambda: {k: np.array(v) for k, v in inp.params.items()}
        torch.cuda.synchronize()
        # 1. warm up on the capture stream
        with torch.cuda.stream(side):
            for _ in range(case.warmups):
                res, _ = case.call(ctx, F, None, side, fresh_params())
        side.synchronize()
        out_g = torch.empty_like(res) if case.takes_out else None
        out_e = torch.empty_like(res) if case.takes_out else None
        own = case.status == "own word"                            # the caller's status word: the caller resets it, no zero-fill in the graph
        if saw:
            saw()
        # 2. capture once, single stream
        params = fresh_params()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            res_g, status_g = case.call(ctx, F, out_g, side, params)
        assert (status_g is not None) == (case.status in ("word", "own word"))
        # 5. the host arrays the call took are overwritten and dropped: a replay uses the captured values
        for a in params.values():
            a.fill(-1)
        del params
        # 3. the mutations, in order
        for k, (label, fields) in enumerate(GR.case_steps(case, inp)):
            what = "%s, replay %d (%s)" % (case.id, k, label)
            for t, h in zip(F, fields):
                t.copy_(torch.from_numpy(np.array(h)))
            _fill_sentinel(torch, res_g)
            if status_g is not None:
                status_g.fill_(0 if own else GR.STATUS_POISON)
            if k == 2:
                noise()                                            # 4. unrelated work on the same pools, on another stream
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = res_g.cpu().numpy()
            st_g = int(status_g.item()) if status_g is not None else (bool(saw()) if saw else None)
            if own:
                status_g.zero_()
            res_e, status_e = case.call(ctx, F, out_e, None, fresh_params())
            torch.cuda.synchronize()
            eager = res_e.cpu().numpy()
            st_e = int(status_e.item()) if status_e is not None else (bool(saw()) if saw else None)
            assert not _has_sentinel(got), what + ": (a) the replay left sentinel words in the result"
            GR.same_bits(got, eager, what + ": (b) replay against the eager call")
            case.compare(inp, got, case.expect(inp, fields), fields, inp.skip if label == "inf" else None)
            assert st_g == st_e, what + ": (d) status %r, the eager call's %r" % (st_g, st_e)
            if case.status != "none":
                assert bool(st_g) == (label == "inf") and (status_g is None or st_g in (0, 1)), what + ": (d) status %r" % (st_g,)
    finally:
        torch.cuda.synchronize()
        del g
        if hasattr(ctx, "close"):
            ctx.close()
