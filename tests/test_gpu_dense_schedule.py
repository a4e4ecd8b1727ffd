"""The schedule of a dense apply (csrc/wagg_dense_route.h: groups of dense_rows_max rows, the ragged split of a group, the
route of each launch) through the real launcher, at the smallest shapes that reach each of its branches:

  fp32  1,369 rows -> 3 x 22 blocks, then 1 x 20   (ragged split)       fp64  400 rows -> 2 x 10, then 1 x 5
          700 rows -> 2 x 22                        (ragged, unsplit)           170 rows -> 1 x 11
          365 rows -> 1 x 23                        (one block: the split form reads the plan's W image)
  65,505 rows (fp32) / 65,473 rows (fp64): one full group of dense_rows_max rows and a group of one row

Results against oracle.ref_numpy.agg_dense on the W read back from the plan, at the tolerances of tests/test_gpu_parity.py.
The result buffer is handed in full of NaN, and the rows on either side of every boundary between launches (and between
row blocks) must come back finite: a wrong row offset of X, of tasmax or of the result shows exactly there.
tests/test_dense_route_host.py pins the schedule itself on the CPU."""
import numpy as np
import pytest

from tests.test_gpu_parity import RTOL32, RTOL64, _rel_ok, torch_cuda  # noqa: F401  (torch_cuda: the parity tests' fixture)

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
RTOL = {F32: RTOL32, F64: RTOL64}
# (dtype, T, G, R, rows on either side of a boundary between launches or row blocks)
FULL = [(F32, 1369, 96, 7, (351, 352, 1055, 1056, 1368)), (F32, 700, 64, 16, (351, 352, 699)), (F32, 365, 96, 7, (0, 364)),
        (F64, 400, 48, 7, (159, 160, 319, 320, 399)), (F64, 170, 48, 7, (0, 169))]
EDGE = [(F32, 65505, 64, 16, (65503, 65504)), (F64, 65473, 32, 16, (65471, 65472))]


def unpack_w(plan, tiles):
    """The (G, R) matrix of a plan from wagg_dense_read_w: stored tile i = `tiles[i]` = (column tile, k tile), a tile
    [256 columns][8 pieces of 16 bytes], piece p of column c at position p ^ ((c >> 1) & 7) (csrc/wagg_dense.hip: tile_slot)."""
    dt = F64 if plan.dtype == "float64" else F32
    E = 16 // np.dtype(dt).itemsize
    bk = 8 * E
    raw = plan.read_w().view(dt).reshape(len(tiles), 256, 8, E)
    c = np.arange(256)[:, None]
    pos = np.arange(8)[None, :] ^ ((c >> 1) & 7)
    by_k = raw[:, c, pos, :].reshape(len(tiles), 256, bk)               # [tile][column][k]
    W = np.zeros((plan.info["n_kt"] * bk, plan.info["n_nt"] * 256), dtype=dt)
    for i, (nt, kt) in enumerate(tiles):
        W[kt * bk:(kt + 1) * bk, nt * 256:(nt + 1) * 256] = by_k[i].T
    assert not W[plan.G:].any() and not W[:, plan.R:].any()             # the padding of G and R is zero
    return W[:plan.G, :plan.R]


def full_tiles(plan):
    return [(nt, kt) for nt in range(plan.info["n_nt"]) for kt in range(plan.info["n_kt"])]


def field(T, G, dtype, seed):
    rng = np.random.default_rng(seed)
    return (280 + 20 * rng.standard_normal((T, G))).astype(dtype)


def apply_checked(torch, plan, run, ref, T, edges, rtol, **tol):
    """`run(out)` into a result buffer full of NaN; every row written, the boundary rows first, then the whole result"""
    out = torch.full((T, plan.R), float("nan"), dtype=torch.float64 if plan.dtype == "float64" else torch.float32, device="cuda")
    got = run(out).cpu().numpy()
    for t in edges:
        assert np.isfinite(got[t]).all(), "row %d" % t
        _rel_ok(got[t], ref[t], rtol, **tol)
    _rel_ok(got, ref, rtol, **tol)
    return got


@pytest.fixture(scope="module")
def full_case(torch_cuda):
    """(plan, read-back W, X, reference) of a full-form case, made once for the tests that share it"""
    from climate_toolbox_amd.engine import DensePlan
    from oracle import ref_numpy as O
    made = {}

    def get(dtype, T, G, R):
        key = (dtype, T, G, R)
        if key not in made:
            plan = DensePlan.synth(G, R, 11, dtype="float64" if dtype == F64 else "float32")
            assert plan.info["form"] == 0 and plan.info["tiled"] == 0
            W = unpack_w(plan, full_tiles(plan))
            np.testing.assert_array_equal(W, O.dense_weights_oracle(G, R, 11).astype(dtype))
            X = field(T, G, dtype, T)
            made[key] = (plan, W, X, O.agg_dense(X, W))
        return made[key]
    return get


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("dtype,T,G,R,edges", FULL + EDGE, ids=lambda v: v.__name__ if isinstance(v, type) else None)
def test_full_form_row_groups(torch_cuda, full_case, dtype, T, G, R, edges, exact):
    torch = torch_cuda
    plan, W, X, ref = full_case(dtype, T, G, R)
    Xd = torch.from_numpy(X).cuda()
    apply_checked(torch, plan, lambda out: plan.apply(Xd, out=out, exact=exact), ref, T, edges, RTOL[dtype])
    assert not plan.saw_inf()


@pytest.mark.parametrize("T,edges", [(365, (0, 364)), (700, (351, 352, 699))])
def test_tile_sparse_row_groups(torch_cuda, T, edges):
    from climate_toolbox_amd.engine import DensePlan
    from oracle import ref_numpy as O
    torch = torch_cuda
    G, R = 64 * 5 + 40, 300                                              # twelve k tiles (one ragged) over two column tiles
    plan = DensePlan.synth_blocklocal(G, R, 5)
    n_kt, n_nt = plan.info["n_kt"], plan.info["n_nt"]
    assert plan.info["tiled"] == 1 and (n_kt, n_nt) == (12, 2) and plan.info["n_tiles"] == n_kt
    # run j of 64 cells (two k tiles) lies in column tile (97 j) mod n_nt; stored in (column tile, k tile) order
    W = unpack_w(plan, sorted(((97 * (kt // 2)) % n_nt, kt) for kt in range(n_kt)))
    np.testing.assert_array_equal(W, O.blocklocal_weights_oracle(G, R, 5))
    X = field(T, G, F32, T)
    Xd = torch.from_numpy(X).cuda()
    ref = O.agg_dense(X, W)
    apply_checked(torch, plan, lambda out: plan.apply(Xd, out=out), ref, T, edges, RTOL32)              # pack-free first pass
    # rows that are not 16-byte aligned take the packed pass alone
    Xo = torch.empty(T * G + 1, dtype=torch.float32, device="cuda")[1:].view(T, G)
    Xo.copy_(Xd)
    apply_checked(torch, plan, lambda out: plan.apply(Xo, out=out), ref, T, edges, RTOL32)


def test_degree_days_across_a_ragged_split(torch_cuda, full_case):
    """tasmax of the tail launch starts `head` rows further down, like tasmin: fp32, 1,369 rows = 1,056 + 313"""
    from oracle import ref_numpy as O
    torch = torch_cuda
    dtype, T, G, R, edges = FULL[0]
    plan, W, X, _ = full_case(dtype, T, G, R)
    Xhi = X + np.random.default_rng(3).uniform(0, 9, X.shape).astype(F32)
    edd = O.snyder_edd_values(X + F32(-273.15), Xhi + F32(-273.15), 14.0)
    Xd, Hd = torch.from_numpy(X).cuda(), torch.from_numpy(Xhi).cuda()
    for exact in (False, True):
        apply_checked(torch, plan, lambda out: plan.apply_edd(Xd, Hd, 14.0, offset=-273.15, out=out, exact=exact), O.agg_dense(edd, W),
                      T, edges, RTOL32, scale=0.05)
    assert not plan.saw_inf()
