"""tests/edd_edges.py checked on the CPU: the catalogue holds every class, the Kelvin variant lands where it claims, the
reference agrees with the oracle, the selected elements equal the oracle's bit for bit, and the derived bound is positive, finite
and holds for an IEEE restatement of the fp32 band expression."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import ref_numpy as O
from tests import edd_edges as EE

DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("e", EE.THRESHOLDS)
def test_catalogue_holds_every_class(dtype, e):
    c = EE.catalogue(dtype, e)
    assert c.tasmin.dtype == dtype and c.tasmax.dtype == dtype and 200 <= len(c.tasmin) <= 400
    for name in EE.CLASSES:
        assert ((c.label == name) & ~c.inf).sum() >= 1, name
    for name in EE.INF_CLASSES:
        assert ((c.label == name) & c.inf).sum() >= 2, name
    assert (c.label == "edge_x_edge").sum() == 25
    assert (c.label == "tmin_edge_partner").sum() == 40 and (c.label == "tmax_edge_partner").sum() == 40
    lo, hi, et = c.tasmin, c.tasmax, dtype(e)
    fin = ~c.inf
    assert np.isfinite(lo[fin] + hi[fin]).sum() >= 200 and not np.isinf(lo[fin]).any() and not np.isinf(hi[fin]).any()
    # what the classes mean, on the values themselves
    for k in EE.ULPS:
        assert ((lo == EE.steps(et, -k, dtype)) & (hi == EE.steps(et, k, dtype)) & (c.label == "edge_x_edge")).sum() == 1
    assert (lo[c.label == "above"] > et).all() and (hi[c.label == "below"] < et).all()
    for name, rel in (("flat_below", np.less), ("flat_above", np.greater)):
        m = c.label == name
        assert (lo[m] == hi[m]).all() and rel(lo[m], et).all()
    m = c.label == "flat_at"
    assert (lo[m] == hi[m]).all() and (lo[m] == et).sum() == 1
    assert (lo[c.label == "inverted"] > hi[c.label == "inverted"]).all()
    m = c.label == "z_0"
    assert np.all(np.abs((hi[m].astype(np.float64) + lo[m]) / 2 - float(et)) <= 2 * np.spacing(np.abs(et)))
    assert np.isnan(lo[c.label == "nan_tmin"]).all() and not np.isnan(hi[c.label == "nan_tmin"]).any()
    m = c.label == "nan_tmax_below"
    assert np.isnan(hi[m]).all() and (lo[m] < et).all()
    m = c.label == "nan_tmax_above"
    assert np.isnan(hi[m]).all() and (lo[m] >= et).all()
    assert np.isnan(lo[c.label == "nan_both"]).all() and np.isnan(hi[c.label == "nan_both"]).all()
    assert np.isposinf(hi[c.label == "inf_tmax"]).all() and np.isneginf(lo[c.label == "inf_tmin"]).all()
    # the selections every kernel has to make are all there, in numbers
    band = EE.in_band(lo, hi, 0.0, e, dtype)
    outer, _ = EE.exact_outer(lo, hi, 0.0, e, dtype)
    assert band.sum() >= 100 and outer.sum() >= 80 and not (band & outer).any()
    assert ((hi == et) & (lo < et)).sum() >= 8 and ((lo == et) & (hi > et)).sum() >= 8
    # widths and |z| are what the class says wherever the type can hold them
    if dtype == np.float64:
        for name, w in zip(("w_2^-20", "w_1", "w_12", "w_40"), EE.WIDTHS):
            m = c.label == name
            np.testing.assert_allclose((hi[m] - lo[m]) / 2, w, rtol=1e-9)
        for name, z in zip(("z_0.5", "z_1-2^-10", "z_1-2^-20"), EE.ZS[1:]):
            m = (c.label == name) & np.isin(c.label, ("z_0.5", "z_1-2^-10", "z_1-2^-20")) & ~c.inf
            m[m] = hi[m] - lo[m] >= 2
            got = np.abs((float(et) - (hi[m] + lo[m]) / 2) / ((hi[m] - lo[m]) / 2))
            np.testing.assert_allclose(1 - got, 1 - z, rtol=1e-6)
            assert band[m].all()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("e", EE.CELSIUS_THRESHOLDS)
def test_kelvin_variant_lands_where_it_claims(dtype, e):
    k = EE.catalogue_kelvin(dtype, e)
    assert k.tasmin.dtype == dtype and len(k.tasmin) == len(EE.catalogue(dtype, e).tasmin)
    assert (k.label == EE.catalogue(dtype, e).label).all()
    lo, hi = EE.moved(k.tasmin, EE.KELVIN, dtype), EE.moved(k.tasmax, EE.KELVIN, dtype)
    fin = np.isfinite(k.tasmin) & np.isfinite(k.tasmax)
    assert (k.tasmin[fin] > 150).all() and (k.tasmax[fin] < 450).all()           # raw Kelvin
    et = dtype(e)
    x_e = EE.raw_for(et, EE.KELVIN, dtype)
    e_land = dtype(x_e + dtype(EE.KELVIN))
    want = Fraction(float(et)) - Fraction(float(dtype(EE.KELVIN)))               # the raw value that would land on e, exactly
    reachable = Fraction(float(dtype(float(want)))) == want
    assert reachable == (e_land == et)
    assert reachable == (e in (-1.75, 8.0, 29.0))                                # 30.3 is not on the grid raw Kelvin data lands on
    assert abs(float(e_land) - float(et)) <= np.spacing(x_e)
    # the edge classes sit k raw steps from the landing of e, after the type's own add
    m = k.label == "edge_x_edge"
    grid = [dtype(EE.steps(x_e, j, dtype) + dtype(EE.KELVIN)) for j in EE.ULPS]
    below = [dtype(EE.steps(x_e, -j, dtype) + dtype(EE.KELVIN)) for j in EE.ULPS]
    assert sorted(set(hi[m].tolist())) == sorted(set(float(g) for g in grid))
    assert sorted(set(lo[m].tolist())) == sorted(set(float(g) for g in below))
    if reachable:
        assert ((hi == et) & (lo < et)).sum() >= 8 and ((lo == et) & (hi > et)).sum() >= 8
        band = EE.in_band(k.tasmin, k.tasmax, EE.KELVIN, e, dtype)
        outer, _ = EE.exact_outer(k.tasmin, k.tasmax, EE.KELVIN, e, dtype)
        assert band.sum() >= 100 and outer.sum() >= 80
    # every other case lands within one raw step of the degree-C case it was made for
    c = EE.catalogue(dtype, e_land)
    far = ~np.isin(k.label, ("edge_x_edge", "tmin_edge_partner", "tmax_edge_partner", "tmin_above_edge", "tmax_below_edge",
                             "nan_tmax_below", "flat_at")) & fin
    assert np.all(np.abs(lo[far].astype(np.float64) - c.tasmin[far]) <= np.spacing(k.tasmin[far]))
    assert np.all(np.abs(hi[far].astype(np.float64) - c.tasmax[far]) <= np.spacing(k.tasmax[far]))


@pytest.mark.parametrize("e", EE.THRESHOLDS)
def test_reference_agrees_with_the_oracle_in_fp64(e):
    c = EE.catalogue(np.float32, e)
    fin = np.isfinite(c.tasmin) & np.isfinite(c.tasmax)
    lo, hi = c.tasmin[fin], c.tasmax[fin]
    ref = EE.reference(lo, hi, 0.0, e, np.float32)
    orc = O.snyder_edd_values(lo.astype(np.float64), hi.astype(np.float64), float(np.float32(e)))
    assert ref.dtype == np.longdouble and not np.isnan(orc).any()
    assert np.max(np.abs(ref - orc)) <= 1e-13
    # ... and the NaN / inf pattern on everything else
    ref_all = EE.reference(c.tasmin, c.tasmax, 0.0, e, np.float32)
    orc_all = O.snyder_edd_values(c.tasmin.astype(np.float64), c.tasmax.astype(np.float64), float(np.float32(e)))
    np.testing.assert_array_equal(np.isnan(ref_all), np.isnan(orc_all))
    np.testing.assert_array_equal(np.isinf(ref_all), np.isinf(orc_all))
    assert np.isnan(ref_all[c.label == "nan_tmax_above"]).all() and (ref_all[c.label == "nan_tmax_below"] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("e", EE.THRESHOLDS)
def test_exact_outer_equals_the_oracle_in_the_data_type(dtype, e):
    for c, off in ((EE.catalogue(dtype, e), 0.0),) + (((EE.catalogue_kelvin(dtype, e), EE.KELVIN),) if e in EE.CELSIUS_THRESHOLDS else ()):
        mask, vals = EE.exact_outer(c.tasmin, c.tasmax, off, e, dtype)
        y_lo, y_hi = EE.moved(c.tasmin, off, dtype), EE.moved(c.tasmax, off, dtype)
        orc = O.snyder_edd_values(y_lo, y_hi, e)
        assert orc.dtype == dtype and vals.dtype == dtype and mask.sum() >= 80
        assert np.array_equal(vals[mask].view(np.uint32 if dtype == np.float32 else np.uint64),
                              orc[mask].view(np.uint32 if dtype == np.float32 else np.uint64))
        rest = ~mask & ~EE.in_band(c.tasmin, c.tasmax, off, e, dtype)            # neither selected nor in band: not finite
        assert not (np.isfinite(c.tasmin[rest]) & np.isfinite(c.tasmax[rest])).any()
        assert (vals[mask & (c.label == "inverted")] != 0).any() and (vals[mask & (c.label == "inverted")] < 0).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_bound_is_positive_and_finite_in_band(dtype):
    for e in EE.THRESHOLDS:
        c = EE.catalogue(dtype, e)
        band = EE.in_band(c.tasmin, c.tasmax, 0.0, e, dtype)
        for form in ("fit32", "fit64", "libm", "ieee"):
            b = EE.bound(c.tasmin[band], c.tasmax[band], e, dtype, form)
            assert np.isfinite(b).all() and (b > 0).all()
            u = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53
            assert (b >= EE.C_BOUND[form] * u * abs(float(dtype(e)))).all()
    assert EE.C_BOUND["ieee"] == 8 and EE.C_BOUND["fit32"] == EE.C_BOUND["fit64"] == 11 and EE.C_BOUND["libm"] == 12


def test_ieee_restatement_of_the_fp32_band_stays_inside_the_bound():
    """A check of the bound, not of the kernel: NumPy float32 with IEEE division and square root, on the catalogue's in-band
    elements and on random in-band pairs, against the reference; c = 8 plus the fit's 5e-9 w."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for e in EE.THRESHOLDS:
        c = EE.catalogue(np.float32, e)
        lo, hi = c.tasmin, c.tasmax
        et = np.float32(e)
        lo = np.concatenate([lo, (et - rng.uniform(0, 30, 400) ** 2 / 30).astype(np.float32)])
        hi = np.concatenate([hi, (et + rng.uniform(0, 30, 400) ** 2 / 30).astype(np.float32)])
        band = EE.in_band(lo, hi, 0.0, e, np.float32)
        got = EE.band_f32_numpy(lo[band], hi[band], e)
        ref = EE.reference(lo[band], hi[band], 0.0, e, np.float32)
        b = EE.bound(lo[band], hi[band], e, np.float32, "ieee") + EE.FIT["fit32"] * (hi[band].astype(np.float64) - lo[band]) / 2
        ratio = np.abs(got - ref) / b
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1).all(), (e, float(ratio.max()))
        assert (got >= 0).all()
    print("IEEE fp32 restatement: max error / bound = %.3f" % worst)


def test_a_wrong_coefficient_would_break_the_bound():
    """the bound is tight enough to matter: P's leading coefficient off by 1e-4 relative is far outside it at w = 10"""
    lo, hi, e = np.array([10.0], np.float32), np.array([30.0], np.float32), 20.0
    ref = EE.reference(lo, hi, 0.0, e, np.float32)
    wrong = float(ref[0]) * (1 + 1e-4)
    assert abs(wrong - float(ref[0])) > 10 * EE.bound(lo, hi, e, np.float32, "fit32")[0]
