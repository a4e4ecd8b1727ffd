"""The plan-owned f16 high / low image of W (csrc/wagg_dense_split.inc: dense_split_image_kernel, and the IMG variant of
dense_split_kernel that loads its operands from it) against the same plan built with WAGG_DENSE_NO_W_IMAGE=1, which splits
W in registers on every apply as before: the same bits, on every route that makes a full-form fp32 plan, for every row-block
shape, k split and transform -- and the image's bytes against the NumPy restatement of the split (tests/split_parts.py)
applied to the packed W.

Shapes: G = 333 (not a whole number of 32-cell k tiles), R = 257 (two column tiles, the second one column and padding);
T = 17 (one row block of 2 x 16), 97 (8 x 16), 350 (22 x 16), 365 (23 x 16), 700 (two row blocks of 22 x 16) and 580 (two
row blocks with a ragged tail, two launches: 20 x 16 rows, then the last 260 in 18 x 16).  Launches of one row block read
the image; with two or more the apply splits in registers on either plan (csrc/wagg_dense.hip: dense_apply_split).
Columns of W: zeros, a largest weight of 2^-149, FLT_MAX, +-inf, NaN, exactly two-part values (hi + lo exact), and the
24-bit weights of split_parts.host_matrix everywhere else."""
import contextlib
import os

import numpy as np
import pytest

from tests import split_parts as S
from tests.test_gpu_parity import torch_cuda  # noqa: F401  (the parity tests' fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32
G, R = 333, 257
ENV = "WAGG_DENSE_NO_W_IMAGE"
COL_ZERO, COL_TINY, COL_FLT_MAX, COL_INF, COL_NAN, COL_TWO_PART = 2, 3, 5, 6, 7, 9
ROUTES = ("host", "csr", "synth", "clone")
ROWS = [(17, 0), (17, 8), (97, 0), (350, 8), (365, 0), (365, 8), (700, 0), (700, 8), (580, 0), (580, 8)]


def matrix(finite_only=False):
    W = np.array(S.host_matrix(G, R))
    W[:, COL_ZERO] = 0.0
    W[:, COL_TINY] = np.where(np.arange(G) % 3 == 0, F32(2.0 ** -149), F32(0.0))
    W[11, COL_FLT_MAX] = S.FLT_MAX
    W[:, COL_TWO_PART] = S.two_part(G).astype(F32)
    if not finite_only:
        W[4, COL_INF], W[200, COL_INF] = np.inf, -np.inf
        W[77, COL_NAN] = np.nan
    assert S.finite_max(W, 0)[COL_TINY] == 2.0 ** -149 and S.finite_max(W, 0)[COL_ZERO] == 0
    return W


@contextlib.contextmanager
def no_image():
    assert ENV not in os.environ
    os.environ[ENV] = "1"
    try:
        yield
    finally:
        del os.environ[ENV]


def _build(route):
    from climate_toolbox_amd.engine import DensePlan
    if route == "host":
        return DensePlan.from_host(matrix())
    if route == "clone":
        src = DensePlan.from_host(matrix())
        try:
            assert src._recipe is None                           # (a plan without a recipe is cloned device to device)
            return src.replica(src.device)
        finally:
            src.close()
    if route == "csr":                                           # a caller's table: the finite non-zero weights, full form forced
        W = matrix(finite_only=True)
        keep = W != 0
        rowptr = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64)
        col = np.nonzero(keep)[1].astype(np.int32)
        return DensePlan.from_csr(rowptr, col, W[keep].astype(np.float64), G, R, form="full")
    return DensePlan.synth(G, R, seed=2)


class _Plans:
    def __init__(self):
        self._p = {}

    def pair(self, route):
        """(the plan built normally, the plan built with the opt-out set)"""
        if route not in self._p:
            a = _build(route)
            with no_image():
                b = _build(route)
            for p in (a, b):
                assert p.info["form"] == 0 and p.dtype == "float32" and p.info["w_bytes"] == 2 * 11 * 32768
            assert a.info["w_image_bytes"] == a.info["w_bytes"], "no image held: %r" % (a.info,)
            assert b.info["w_image_bytes"] == 0
            self._p[route] = (a, b)
        return self._p[route]

    def close(self):
        for a, b in self._p.values():
            a.close()
            b.close()


@pytest.fixture(scope="module")
def plans(torch_cuda):  # noqa: F811
    p = _Plans()
    yield p
    p.close()


@pytest.fixture(scope="module")
def fields(torch_cuda):  # noqa: F811
    """(tasmin-like X, tasmax) of 700 rows on the device: kelvin values, rows of very different magnitude, some NaN"""
    rng = np.random.default_rng(333)
    X = rng.uniform(250.0, 310.0, (700, G)).astype(F32)
    X[::7] *= F32(2.0 ** -20)
    X[3::11] *= F32(2.0 ** 30)
    X[rng.random((700, G)) < 0.01] = np.nan
    X2 = X + rng.uniform(0.0, 15.0, (700, G)).astype(F32)
    return torch_cuda.from_numpy(X).cuda(), torch_cuda.from_numpy(X2).cuda()


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return np.array_equal(a, b), "%d of %d words differ" % (int((a != b).sum()), a.size)


@pytest.mark.parametrize("T,ksplit", ROWS, ids=["T%d-ks%d" % c for c in ROWS])
@pytest.mark.parametrize("route", ROUTES)
def test_apply_bits(plans, fields, route, T, ksplit):
    a, b = plans.pair(route)
    X = fields[0][:T]
    ok, msg = _same_bits(a.apply(X, ksplit=ksplit), b.apply(X, ksplit=ksplit))
    assert ok, msg


@pytest.mark.parametrize("T", [17, 365, 700, 580])
@pytest.mark.parametrize("what", ["poly2", "edd"])
def test_transform_bits(plans, fields, what, T):
    a, b = plans.pair("host")
    X, X2 = fields[0][:T], fields[1][:T]
    if what == "poly2":
        ra, rb = a.apply_poly(X, -273.15, 2), b.apply_poly(X, -273.15, 2)
    else:
        ra, rb = a.apply_edd(X, X2, 29.0, offset=-273.15), b.apply_edd(X, X2, 29.0, offset=-273.15)
    ok, msg = _same_bits(ra, rb)
    assert ok, msg


def test_clone_follows_the_rule(plans):
    """a clone decides by the rule of a first build on its own device, whatever its source holds: no image with the opt-out
    set at the time of the clone, one without it"""
    a, b = plans.pair("host")
    with no_image():
        c = a.replica(a.device)
    d = b.replica(b.device)
    try:
        assert c.info["w_image_bytes"] == 0 and d.info["w_image_bytes"] == d.info["w_bytes"]
    finally:
        c.close()
        d.close()


def test_other_plans_hold_no_image(torch_cuda):  # noqa: F811
    from climate_toolbox_amd.engine import DensePlan
    W = matrix(finite_only=True)
    for p in (DensePlan.from_host(W.astype(np.float64)), DensePlan.synth_blocklocal(4096, 600, seed=3),
              DensePlan.synth(4096, 300, seed=3, fill=0.01)):
        try:
            assert p.info["w_image_bytes"] == 0, p.info
        finally:
            p.close()


def test_exact_apply_reads_fp32_w(plans, fields):
    """the exact kernel reads the fp32 W of either plan: the same bits"""
    a, b = plans.pair("host")
    ok, msg = _same_bits(a.apply(fields[0][:17], exact=True), b.apply(fields[0][:17], exact=True))
    assert ok, msg


def test_image_bytes(torch_cuda):  # noqa: F811
    """The image of a 333 x 257 plan, slot by slot: lane (lr, kq) of wave w owns the 16-byte slots at w 4096 + frag0 / frag1
    (+ 2048 for its second column) of every 32-KiB tile; the image holds at frag0 the eight f16 high parts and at frag1 the
    eight low parts of the eight scaled weights that the packed W holds at frag0 | frag1.  A weight that is +-inf or NaN is
    not cleaned as a cell of X is (split_parts.parts): split_w8 keeps hi = f16(w) and lo = f16(w - hi) = NaN; which NaN is
    not pinned, every other half is compared bit for bit."""
    from climate_toolbox_amd.engine import DensePlan
    W = matrix()
    p = DensePlan.from_host(W)
    try:
        assert p.info["w_image_bytes"] == p.info["w_bytes"]
        n_kt, n_nt = p.info["n_kt"], p.info["n_nt"]
        packed = p.read_w().view(F32).reshape(n_nt, n_kt, 8, 4096 // 4)     # [column tile][k tile][wave][floats]
        image = p.read_w(image=True).view(np.uint16).reshape(n_nt, n_kt, 8, 4096 // 2)
    finally:
        p.close()
    wmax = np.zeros(n_nt * 256)
    wmax[:R] = S.finite_max(W, 0)
    ew = S.split_exp(wmax).reshape(n_nt, 1, 8, 2, 16)            # [column tile][.][wave][column block][lr]
    want = np.zeros_like(image)
    cells = 0
    for lr in range(16):
        for kq in range(4):
            f0 = lr * 8 + (kq ^ (lr >> 1))                       # in 16-byte slots
            f1 = lr * 8 + ((kq ^ (lr >> 1)) ^ 4)
            for cb in range(2):
                s0, s1 = f0 + 128 * cb, f1 + 128 * cb
                v = np.concatenate([packed[..., 4 * s0:4 * s0 + 4], packed[..., 4 * s1:4 * s1 + 4]], axis=-1)
                hi, lo = S.parts(v, ew[:, :, :, cb, lr][..., None])
                hi = np.where(np.isnan(v), np.nan, hi)
                lo = np.where(np.isfinite(v), lo, np.nan)
                want[..., 8 * s0:8 * s0 + 8] = hi.astype(np.float16).view(np.uint16)
                want[..., 8 * s1:8 * s1 + 8] = lo.astype(np.float16).view(np.uint16)
                cells += v.size
    assert cells == packed.size and image.size == 2 * cells      # every slot of a tile belongs to one lane
    # the packed W is the matrix: column 32 w + 16 cb + lr of a tile, k = 4 kq + c and 16 + 4 kq + c of its k tile
    k0 = 4 * 1
    assert packed[0, 0, 0, 4 * (3 * 8 + (1 ^ (3 >> 1))):][:4].tolist() == W[k0:k0 + 4, 3].tolist()
    want_nan = np.isnan(want.view(np.float16))
    assert want_nan.sum() == 1 + 2 + 1                           # NaN: hi and lo; +-inf: lo
    bad = np.where(want_nan, ~np.isnan(image.view(np.float16)), want != image)
    assert not bad.any(), "%d of %d halves differ, first at %r" % (int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))
