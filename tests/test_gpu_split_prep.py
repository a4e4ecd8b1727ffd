"""The two kernels that prepare X for the split apply (csrc/wagg_dense_split.inc): dense_rowmax_kernel, which writes 64 per-strip
maxima a row, and dense_pack_x_split_kernel, which folds them, leaves the row maxima for the reduce and writes the packed f16
high / low tiles, one thread per pair of pieces.  The packed bytes and the row maxima are read back (DensePlan.read_split) and
compared bit for bit with the packer restated from tests/split_parts.py (`image`): row t scaled by 2^ex[t], ex from the row's
largest finite |x|; piece p < 4 of a tile row holds the high parts and piece p + 4 the low parts of cells 4 p + c and
16 + 4 p + c of the k tile, stored at slot piece ^ ((row >> 1) & 7); rows past T and cells past G are zero.

Shapes: G from 1 to 64 x 4096 + 5 -- fewer, as many and more cells than 64 strips of one 4-cell piece, a ragged last piece, and
at the largest G strips long enough for the row-maximum kernel's unrolled loop (1,025 pieces a strip) -- against T = 1, 15, 16, 17
(one or two 16-row groups, full or ragged), and T = 365 (the tallest row block, 23 x 16) at G = 257.  All launches have one row
block; launches of several run the same kernels with another grid and are covered by tests/test_gpu_split_image.py (T = 700,
580) through the result."""
import numpy as np
import pytest

from tests import split_parts as S
from tests.test_gpu_parity import torch_cuda  # noqa: F401  (the parity tests' fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32
R = 3
MTS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 14, 16, 18, 20, 21, 22, 23)  # csrc/wagg_dense_route.h: the fp32 row-block heights
GS = (1, 3, 31, 32, 33, 4095, 4096, 4097, 64 * 4096 + 5)
TS = (1, 15, 16, 17)
SHAPES = [(T, G) for G in GS for T in TS] + [(365, 257)]
OFFSET = -273.15


def image(Y):
    """(packed tiles as uint16 [k tile][tile row][slot][8], row maxima as fp32) of a field Y (T, G) that is already transformed"""
    Y = np.asarray(Y, dtype=F32)
    T, G = Y.shape
    bm = 16 * next(m for m in MTS if 16 * m >= T)
    n_kt = -(-G // 32)
    m = S.finite_max(Y, 1)
    pad = np.zeros((bm, n_kt * 32))
    pad[:T, :G] = Y
    ex = np.zeros(bm, dtype=np.int64)
    ex[:T] = S.split_exp(m)
    hi, lo = S.parts(pad, ex[:, None])
    pieces = []
    for part in (hi, lo):                                        # cell 16 half + 4 p + c of a k tile -> piece p, element 4 half + c
        a = part.reshape(bm, n_kt, 2, 4, 4).transpose(1, 0, 3, 2, 4).reshape(n_kt, bm, 4, 8)
        pieces.append(a.astype(np.float16).view(np.uint16))
    pieces = np.concatenate(pieces, axis=2)                      # [k tile][row][piece 0..7][8]
    row = np.arange(bm)[:, None]
    slot = np.arange(8)[None, :]
    want = pieces[:, row, slot ^ ((row >> 1) & 7)]               # slot s of a row holds piece s ^ swizzle
    return want, m.astype(F32)


def field(T, G, seed=0):
    """rows of very different magnitude, both signs, 2 % NaN; the largest |x| of a row wherever it falls"""
    rng = np.random.default_rng(1000 * T + G + seed)
    X = (rng.uniform(-1.0, 1.0, (T, G)) * 2.0 ** rng.integers(-30, 31, (T, 1))).astype(F32)
    X[rng.random((T, G)) < 0.02] = np.nan
    return X


class _Ctx:
    def __init__(self, torch):
        self.torch, self._plans = torch, {}

    def weights(self, G):
        return np.random.default_rng(G).uniform(0.25, 1.0, (G, R)).astype(F32)

    def fresh(self, G):
        from climate_toolbox_amd.engine import DensePlan
        p = DensePlan.from_host(self.weights(G))
        assert p.info["form"] == 0 and p.dtype == "float32"
        return p

    def plan(self, G):
        if G not in self._plans:
            self._plans[G] = self.fresh(G)
        return self._plans[G]

    def dev(self, a):
        return self.torch.from_numpy(np.array(a, order="C")).cuda()

    def view(self, X, way):
        """X on the device: "contiguous"; "pitched" (16-byte aligned rows, NaN in the pad); "offset" (one element into that
        buffer); "odd" (a row stride of an odd number of elements)"""
        torch, (T, G) = self.torch, X.shape
        Xd = self.dev(X)
        if way == "contiguous":
            return Xd
        pitch = (G + 8) // 4 * 4 + (1 if way == "odd" else 0)
        c0 = 1 if way == "offset" else 0
        wide = torch.full((T, pitch), float("nan"), dtype=Xd.dtype, device="cuda")
        wide[:, c0:c0 + G] = Xd
        v = wide[:, c0:c0 + G]
        aligned = v.data_ptr() % 16 == 0 and (v.stride(0) * v.element_size()) % 16 == 0
        assert aligned == (way == "pitched")
        return v

    def read(self, plan, T, G):
        """(packed tiles, row maxima) as the last apply of T rows left them"""
        self.torch.cuda.synchronize()
        bm = 16 * next(m for m in MTS if 16 * m >= T)
        n_kt = -(-G // 32)
        xp = plan.read_split("xp", n_kt * bm * 128).view(np.uint16).reshape(n_kt, bm, 8, 8)
        return xp, plan.read_split("xmax", 4 * T).view(F32)

    def close(self):
        for p in self._plans.values():
            p.close()


@pytest.fixture(scope="module")
def ctx(torch_cuda):  # noqa: F811
    c = _Ctx(torch_cuda)
    yield c
    c.close()


def _same(got, want, what):
    (xp, xmax), (wp, wmax) = got, want
    assert np.array_equal(xmax.view(np.uint32), wmax.view(np.uint32)), "%s: row maxima %r, expected %r" % (what, xmax, wmax)
    bad = xp != wp
    assert not bad.any(), "%s: %d of %d halves differ, first at [k tile, row, slot, c] = %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


@pytest.mark.parametrize("T,G", SHAPES, ids=["T%d-G%d" % s for s in SHAPES])
def test_packed_image(ctx, T, G):
    X = field(T, G)
    plan = ctx.plan(G)
    plan.apply(ctx.dev(X))
    _same(ctx.read(plan, T, G), image(X), "T = %d, G = %d" % (T, G))
    assert not plan.saw_inf()


@pytest.mark.parametrize("G", GS)
def test_layouts(ctx, G):
    """pitched and aligned, one element into the buffer, an odd row stride: the bits of contiguous rows, image and result"""
    T = 17
    X = field(T, G, seed=1)
    plan = ctx.plan(G)
    first = plan.apply(ctx.view(X, "contiguous")).cpu().numpy()
    want = ctx.read(plan, T, G)
    _same(want, image(X), "contiguous")
    for way in ("pitched", "offset", "odd"):
        got = plan.apply(ctx.view(X, way)).cpu().numpy()
        _same(ctx.read(plan, T, G), want, way)
        assert np.array_equal(got.view(np.uint32), first.view(np.uint32)), way


SPECIAL = ("max in the first strip", "max in the last cell", "max in a middle strip", "zeros", "NaN", "+inf", "-inf", "FLT_MAX",
           "subnormals", "-0.0")


@pytest.mark.parametrize("way", ["contiguous", "odd"])
@pytest.mark.parametrize("G", [4097, 64 * 4096 + 5])
def test_special_values(ctx, G, way):
    """One row a case of SPECIAL.  A row with +-inf: the high part of that cell is +-inf, its low part 0, the row's scale that of
    its largest finite value, and the plan's note is set; FLT_MAX and a row of subnormals alone are scaled like any other."""
    rng = np.random.default_rng(G)
    X = rng.uniform(-0.5, 0.5, (len(SPECIAL), G)).astype(F32)
    X[0, 0] = 1000.0
    X[1, G - 1] = -1000.0                                        # (the ragged last piece: G % 4 = 1)
    X[2, G // 2 + 1] = 1000.0
    X[3] = 0.0
    X[4] = np.nan
    X[5, 5], X[5, G // 3] = np.inf, 7.0
    X[6, G - 2] = -np.inf
    X[7] *= F32(2.0 ** 100)
    X[7, 77] = -S.FLT_MAX
    X[8] = (rng.integers(-2 ** 22, 2 ** 22, G) * 2.0 ** -149).astype(F32)
    X[8, G - 3] = F32(2.0 ** -127)
    X[9] = -0.0
    want, m = image(X)
    assert m[0] == m[1] == m[2] == 1000 and m[3] == m[4] == m[9] == 0 and m[5] == 7 and m[6] <= 0.5 and m[7] == S.FLT_MAX
    assert m[8] == 2.0 ** -127
    plan = ctx.plan(G)
    assert not plan.saw_inf()
    plan.apply(ctx.view(X, way))
    got = ctx.read(plan, len(SPECIAL), G)
    _same(got, (want, m), way)
    assert plan.saw_inf() and not plan.saw_inf()
    # the +inf cell itself: row 5, cell 5 = k tile 0, piece 1 (high) and 5 (low), element 1; swizzle of row 5 is 2
    assert got[0][0, 5, 1 ^ 2, 1] == 0x7C00 and got[0][0, 5, 5 ^ 2, 1] == 0


def test_transforms(ctx):
    """apply_poly and apply_edd pack the library's own element transform of the field (engine.transform_poly / transform_edd,
    pinned by test_gpu_element_ops and test_gpu_edd_edges): the same bits as the restatement applied to that"""
    from climate_toolbox_amd import engine
    T, G = 17, 333
    rng = np.random.default_rng(9)
    X = rng.uniform(250.0, 310.0, (T, G)).astype(F32)
    X[rng.random((T, G)) < 0.02] = np.nan
    X2 = X + rng.uniform(0.0, 15.0, (T, G)).astype(F32)
    plan = ctx.plan(G)
    for way in ("contiguous", "odd"):
        Xd, X2d = ctx.view(X, way), ctx.view(X2, way)
        Y = engine.transform_poly(ctx.dev(X), OFFSET, 2).cpu().numpy().reshape(T, G)
        plan.apply_poly(Xd, OFFSET, 2)
        _same(ctx.read(plan, T, G), image(Y), "poly, " + way)
        Y = engine.transform_edd(ctx.dev(X), ctx.dev(X2), OFFSET, [(1.0, 29.0)]).cpu().numpy().reshape(T, G)
        assert (Y[np.isfinite(Y)] > 0).any()
        plan.apply_edd(Xd, X2d, 29.0, offset=OFFSET)
        _same(ctx.read(plan, T, G), image(Y), "edd, " + way)


@pytest.mark.parametrize("G", [33, 4097, 64 * 4096 + 5])
def test_no_stale_partials(ctx, G):
    """field A, then field B with smaller maxima in every strip, on one plan: B's row maxima, image and result are those of B on
    a fresh plan, bit for bit"""
    T = 17
    B = field(T, G, seed=2)
    A = np.where(np.isnan(B), F32(3.0), B) * F32(2.0 ** 40) + F32(1.0)
    assert (S.finite_max(A, 1) > S.finite_max(B, 1)).all()
    fresh = ctx.fresh(G)
    try:
        want = fresh.apply(ctx.dev(B)).cpu().numpy()
        want_ws = ctx.read(fresh, T, G)
    finally:
        fresh.close()
    plan = ctx.plan(G)
    plan.apply(ctx.dev(A))
    got = plan.apply(ctx.dev(B)).cpu().numpy()
    _same(ctx.read(plan, T, G), want_ws, "B after A")
    _same(want_ws, image(B), "B on a fresh plan")
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
