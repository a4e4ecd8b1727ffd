"""Many-plans on the GPU (wagg_plan_create_many, engine.ManyPlan): {popwt, areawt} x {hierid, ISO} of the c2-real / c3 tables
from one pass over the field -- fine planes bit for bit the single plans, ISO derived from the hierid partial sums."""
import time

import numpy as np
import pytest

from tests.test_gpu_parity import RTOL32, RTOL64, _rel_ok

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


@pytest.fixture(scope="module")
def c2_table():
    from climate_toolbox_amd import synth
    lat, lon, df = synth.realistic_segments()           # 720 x 1440, R = 24,378
    pop = synth.code_segments(df, lat, lon, "popwt", "hierid")
    area = synth.code_segments(df, lat, lon, "areawt", "hierid")
    _, _, _, iso_u = synth.code_segments(df, lat, lon, "areawt", "ISO")
    iso = synth.code_segments(df, lat, lon, "areawt", "ISO")[1]
    np.testing.assert_array_equal(pop[0], area[0])
    return dict(lat=lat, lon=lon, cell=area[0], hier=area[1], R=len(area[3]), iso=iso, R_iso=len(iso_u),
                w=[pop[2], area[2]], G=len(lat) * len(lon))


def _field(dtype, T, G, seed=11):
    from climate_toolbox_amd import engine
    return engine.synth_field(T, G, seed=seed, base=280.0, amp=60.0, dtype="float64" if dtype == np.float64 else "float32")


@pytest.mark.parametrize("dtype,rtol,tol_sep", [(np.float32, RTOL32, 1e-5), (np.float64, RTOL64, 1e-12)])
def test_many_vs_single_plans_full_size(torch_cuda, c2_table, dtype, rtol, tol_sep):
    from climate_toolbox_amd import _lib, engine
    from oracle import ref_numpy as O
    t = c2_table
    G, T = t["G"], 365
    X = _field(dtype, T, G)
    many = engine.ManyPlan(t["cell"], t["hier"], t["w"], G, t["R"], row_len=len(t["lon"]), levels=[(t["iso"], t["R_iso"])])
    assert many.out_cols == 2 * t["R"] + 2 * t["R_iso"]
    engine.profile_enable(True)
    views = many.apply(X)
    torch_cuda.cuda.synchronize()
    assert len(engine.profile_read()) == 1, "one dominant kernel = one pass over X for both weightings"
    engine.profile_enable(False)
    dev = [[v.cpu().numpy() for v in row] for row in views]
    Xh = X.cpu().numpy()
    for k, w in enumerate(t["w"]):
        single = engine.SparsePlan(t["cell"], t["hier"], w, G, t["R"], row_len=len(t["lon"]))
        np.testing.assert_array_equal(dev[0][k], single.apply(X).cpu().numpy())
        np.testing.assert_array_equal(many.den[0][k], single.den)
        sep = engine.SparsePlan(t["cell"], t["iso"], w, G, t["R_iso"], row_len=len(t["lon"]))
        np.testing.assert_array_equal(many.den[1][k], sep.den)            # coarse den bit for bit a plan over the coarse codes
        ref = O.agg_coded(Xh, t["cell"], t["iso"], w, t["R_iso"])
        _rel_ok(dev[1][k], ref, rtol)
        s = sep.apply(X).cpu().numpy().astype(np.float64)
        d = np.abs(dev[1][k] - s) / np.maximum(np.abs(s), 1e-300)
        print("ISO derived vs separate plan (%s, weighting %d): max rel diff %.3e" % (np.dtype(dtype).name, k, d.max()))
        assert d.max() <= tol_sep
        single.close(); sep.close()
    # (region, time) results of the same plan: the same numbers
    rt = many.apply(X, out_layout="RT")
    for l in range(2):
        for k in range(2):
            np.testing.assert_array_equal(rt[l][k].cpu().numpy().T, dev[l][k])
    # host-resident field: one call, one crossing, the device bits
    _lib.host_stats(reset=True)
    host = many.apply_host(Xh, flags=_lib.HOST_PIN | _lib.HOST_LINES)
    st_many = _lib.host_stats(reset=True)
    for l in range(2):
        for k in range(2):
            np.testing.assert_array_equal(host[l][k], dev[l][k])
    single = engine.SparsePlan(t["cell"], t["hier"], t["w"][0], G, t["R"], row_len=len(t["lon"]))
    single.apply_host(Xh, flags=_lib.HOST_PIN | _lib.HOST_LINES)
    st_one = _lib.host_stats(reset=True)
    assert st_many["lines_h2d_bytes"] == st_one["lines_h2d_bytes"] > 0
    single.close(); many.close()


@pytest.mark.parametrize("dtype,K,passes", [(np.float32, 4, 1), (np.float64, 4, 2), (np.float64, 3, 2)])
def test_many_weightings_per_pass(torch_cuda, c2_table, dtype, K, passes):
    from climate_toolbox_amd import engine
    t = c2_table
    G, T = t["G"], 100
    X = _field(dtype, T, G, seed=3)
    rng = np.random.default_rng(5)
    ws = [t["w"][0], t["w"][1]] + [rng.uniform(0.1, 1, len(t["cell"])) for _ in range(K - 2)]
    many = engine.ManyPlan(t["cell"], t["hier"], ws, G, t["R"], row_len=len(t["lon"]))
    engine.profile_enable(True)
    views = many.apply(X)
    torch_cuda.cuda.synchronize()
    assert len(engine.profile_read()) == passes
    engine.profile_enable(False)
    for k in range(K):
        single = engine.SparsePlan(t["cell"], t["hier"], ws[k], G, t["R"], row_len=len(t["lon"]))
        np.testing.assert_array_equal(views[0][k].cpu().numpy(), single.apply(X).cpu().numpy())
        single.close()
    many.close()


def test_many_edge_cases(torch_cuda):
    from climate_toolbox_amd import _lib, engine, synth
    from oracle import ref_numpy as O
    torch = torch_cuda
    lat, lon, df = synth.realistic_segments(nlat=180, nlon=360, R=600, n_iso=30, seed=4, string_labels=False)
    cell, hier, pop, _ = synth.code_segments(df, lat, lon, "popwt", "hierid")
    _, _, area, _ = synth.code_segments(df, lat, lon, "areawt", "hierid")
    _, iso, _, iso_u = synth.code_segments(df, lat, lon, "areawt", "ISO")
    G, R, R_iso = len(lat) * len(lon), int(hier.max()) + 1, len(iso_u) + 1      # one more ISO code: an empty coarse region
    area = area.copy()
    area[np.flatnonzero(pop > 0)[::5]] = np.nan          # kept rows diverge between the weightings
    for dtype, rtol in ((np.float32, RTOL32), (np.float64, RTOL64)):
        many = engine.ManyPlan(cell, hier, [pop, area], G, R, row_len=len(lon), levels=[(iso, R_iso)])
        for T in (1, 100):
            X = _field(dtype, T, G, seed=T)
            v = many.apply(X)
            Xh = X.cpu().numpy()
            for k, w in enumerate((pop, area)):
                wk = w if k == 0 else np.where(np.isnan(area), 0.0, area)   # NaN on a row the other keeps = weight 0
                _rel_ok(v[0][k].cpu().numpy(), O.agg_coded(Xh, cell, hier, wk, R), rtol)
                _rel_ok(v[1][k].cpu().numpy(), O.agg_coded(Xh, cell, iso, wk, R_iso), rtol)
                assert np.isnan(v[1][k].cpu().numpy()[:, -1]).all()         # empty coarse region: 0 / 0
        # K = 1, L = 0: a wagg_plan_create plan, bit for bit
        one = engine.ManyPlan(cell, hier, [pop], G, R, row_len=len(lon))
        single = engine.SparsePlan(cell, hier, pop, G, R, row_len=len(lon))
        X = _field(dtype, 365, G, seed=9)
        assert torch.equal(one.apply(X)[0][0], single.apply(X))
        # a fused transform on a many-plan is refused
        with pytest.raises(_lib.WaggError) as e:
            _lib.run("poly", plan_kind=_lib.PLAN_SEGMENT, plan=many._h, elem=engine._elem(X.dtype), source=_lib.SRC_DEVICE,
                     transform=_lib.XF_POLY, offset=0.0, pow_first=1, n_pow=1, x=X.data_ptr(), T=365, ldx=G,
                     out=X.data_ptr(), ldo=many.out_cols, out_pstride=0)
        assert e.value.code == -5
        # no whole-line chunking (no row length): weightings run one after the other, derived levels are refused
        flat = engine.ManyPlan(cell, hier, [pop, area], G, R)
        fv = flat.apply(X)
        flat_single = engine.SparsePlan(cell, hier, pop, G, R)
        assert torch.equal(fv[0][0], flat_single.apply(X))
        flat_single.close()
        with pytest.raises(_lib.WaggError):
            engine.ManyPlan(cell, hier, [pop], G, R, levels=[(iso, R_iso)]).apply(X)
        many.close(); one.close(); single.close(); flat.close()


def test_reference_fixture_many_gt_layout(torch_cuda, ref_fixture):
    """The reference's fixture ((lat, lon, time): GT layout, so the weightings run one after the other) through one
    many-plan: both weightings against the golden expectations."""
    from climate_toolbox_amd import engine
    from climate_toolbox_amd.aggregations import _backup_fill, _factorize_labels, _resolve_cells
    torch = torch_cuda
    fx, gold = ref_fixture
    cell = _resolve_cells(fx["lat"], fx["lon"], fx["seg_lat"], fx["seg_lon"])
    uniq, codes = _factorize_labels(fx["ISO"])
    ws = [_backup_fill(fx["popwt"], fx["areawt"]), _backup_fill(fx["areawt"], fx["areawt"])]
    G = len(fx["lat"]) * len(fx["lon"])
    X = torch.from_numpy(np.ascontiguousarray(fx["temp"].reshape(G, -1))).cuda()
    many = engine.ManyPlan(cell, codes, ws, G, len(uniq))
    v = many.apply(X, layout="GT", out_layout="RT")
    for k, name in enumerate(("popwt", "areawt")):
        single = engine.SparsePlan(cell, codes, ws[k], G, len(uniq))
        assert torch.equal(v[0][k], single.apply(X, layout="GT", out_layout="RT"))
        _rel_ok(v[0][k].cpu().numpy(), gold["expect_%s_ISO" % name], RTOL64)
        single.close()
    many.close()


def test_zz_many_host_perf_guard(torch_cuda, c2_table):
    """One host-resident many call for the four combinations <= 0.5 x the four single host calls (two interleaved rounds,
    the lower median per form)."""
    from climate_toolbox_amd import _lib, engine
    t = c2_table
    G, T = t["G"], 365
    Xh = _field(np.float32, T, G).cpu().numpy()
    flags = _lib.HOST_PIN | _lib.HOST_LINES
    many = engine.ManyPlan(t["cell"], t["hier"], t["w"], G, t["R"], row_len=len(t["lon"]), levels=[(t["iso"], t["R_iso"])])
    singles = [engine.SparsePlan(t["cell"], c, w, G, r, row_len=len(t["lon"]))
               for w in t["w"] for c, r in ((t["hier"], t["R"]), (t["iso"], t["R_iso"]))]
    many.apply_host(Xh, flags=flags)
    for s in singles:
        s.apply_host(Xh, flags=flags)
    med = {"many": [], "four": []}
    for _ in range(2):
        a, b = [], []
        for _ in range(5):
            t0 = time.perf_counter(); many.apply_host(Xh, flags=flags); a.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for s in singles:
                s.apply_host(Xh, flags=flags)
            b.append(time.perf_counter() - t0)
        med["many"].append(np.median(a)); med["four"].append(np.median(b))
    m, f = min(med["many"]), min(med["four"])
    print("host-resident c2-real fp32: one many call %.2f ms, four single calls %.2f ms (ratio %.2f)" % (1e3 * m, 1e3 * f, m / f))
    assert m <= 0.5 * f
    many.close()
    for s in singles:
        s.close()


def _ds_table(dtype, on_device, T=40, seed=4):
    import pandas as pd
    import torch
    from climate_toolbox_amd import minixr, synth
    lat, lon, df = synth.realistic_segments(nlat=180, nlon=360, R=600, n_iso=30, seed=seed, string_labels=True)
    rng = np.random.default_rng(seed)
    vals = (280 + 20 * rng.standard_normal((T, len(lat), len(lon)))).astype(dtype)
    if on_device:
        vals = torch.from_numpy(vals).cuda()
    ds = minixr.Dataset({"tas": (("time", "lat", "lon"), vals)}, coords={"time": np.datetime64("2001-01-01") + np.arange(T), "lat": lat, "lon": lon})
    return ds, pd.DataFrame(df)


COMBOS = [("popwt", "hierid"), ("areawt", "hierid"), ("popwt", "ISO"), ("areawt", "ISO")]


def _same_as_single(got, ds, df, variable, rtol_iso):
    from climate_toolbox_amd import weighted_aggregate_grid_to_regions
    assert list(got) == COMBOS
    for (aggwt, agglev), out in got.items():
        ref = weighted_aggregate_grid_to_regions(ds, variable, aggwt, agglev, df)
        assert out[variable].dims == ref[variable].dims
        assert list(out.coords) == list(ref.coords)
        np.testing.assert_array_equal(out[agglev].values, ref[agglev].values)
        np.testing.assert_array_equal(out["time"].values, ref["time"].values)
        a, b = np.asarray(out[variable].values), np.asarray(ref[variable].values)
        if agglev == "hierid":
            np.testing.assert_array_equal(a, b)
        else:
            np.testing.assert_allclose(a, b, rtol=rtol_iso, atol=0)


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("dtype,rtol_iso", [(np.float32, 1e-5), (np.float64, 1e-12)])
def test_dataset_many_matches_single_calls(torch_cuda, dtype, rtol_iso, on_device):
    from climate_toolbox_amd import _lib, engine, weighted_aggregate_grid_to_regions_many
    from climate_toolbox_amd._plans import _PLAN_CACHE
    from climate_toolbox_amd.engine import ManyPlan
    ds, df = _ds_table(dtype, on_device)
    _lib.host_stats(reset=True)
    got = weighted_aggregate_grid_to_regions_many(ds, "tas", COMBOS, df)
    st = _lib.host_stats(reset=True)
    if not on_device:
        assert st["calls"] == 1, st                      # one host pipeline call for all four
    many = [p for p in _PLAN_CACHE.values() if isinstance(p, ManyPlan)]
    assert len(many) >= 1 and any(p.n_levels == 1 and p.n_weights == 2 for p in many)
    # the second call takes the cached many-plan
    n = len(_PLAN_CACHE)
    engine.profile_enable(True)
    weighted_aggregate_grid_to_regions_many(ds, "tas", COMBOS, df)
    torch_cuda.cuda.synchronize()
    if on_device:
        assert len(engine.profile_read()) == 1           # one pass over X for the four
    engine.profile_enable(False)
    assert len(_PLAN_CACHE) == n
    _same_as_single(got, ds, df, "tas", rtol_iso)


def test_dataset_many_results_on_device(torch_cuda):
    from climate_toolbox_amd import results_on_device, weighted_aggregate_grid_to_regions_many
    ds, df = _ds_table(np.float32, True)
    with results_on_device():
        got = weighted_aggregate_grid_to_regions_many(ds, "tas", COMBOS, df)
        assert all(torch_cuda.is_tensor(o["tas"].data) and o["tas"].data.is_cuda for o in got.values())
        host = {k: np.asarray(o["tas"].values) for k, o in got.items()}          # (.values copies out on demand)
    ref = weighted_aggregate_grid_to_regions_many(ds, "tas", COMBOS, df)
    for k in COMBOS:
        np.testing.assert_array_equal(host[k], np.asarray(ref[k]["tas"].values))


def test_dataset_many_reference_fixture(torch_cuda, ref_fixture):
    """(lat, lon, time) fixture: GT layout, so ISO and hierid are separate many-plans; against the golden values."""
    import pandas as pd
    from climate_toolbox_amd import minixr, weighted_aggregate_grid_to_regions_many
    fx, gold = ref_fixture
    df = pd.DataFrame({k: fx[s] for k, s in (("lat", "seg_lat"), ("lon", "seg_lon"), ("areawt", "areawt"), ("popwt", "popwt"),
                                              ("ISO", "ISO"), ("hierid", "hierid"))})
    ds = minixr.Dataset({"temperature": (["lat", "lon", "time"], fx["temp"])},
                        coords={"lon": fx["lon"], "lat": fx["lat"], "time": np.arange(10)})
    got = weighted_aggregate_grid_to_regions_many(ds, "temperature", COMBOS, df)
    for (aggwt, agglev), out in got.items():
        assert out.temperature.dims == (agglev, "time")
        _rel_ok(out.temperature.values, gold["expect_%s_%s" % (aggwt, agglev)], RTOL64)


def test_dataset_many_weights_from_csv(torch_cuda, tmp_path):
    """The weights given as the path of a CSV take the reference's loading route: the same results as the DataFrame."""
    from climate_toolbox_amd import weighted_aggregate_grid_to_regions_many
    ds, df = _ds_table(np.float32, False, T=20)
    csv = tmp_path / "w.csv"
    df.rename(columns={"lon": "pix_cent_x", "lat": "pix_cent_y"}).to_csv(csv, index=False)
    got = weighted_aggregate_grid_to_regions_many(ds, "tas", COMBOS, df)
    got2 = weighted_aggregate_grid_to_regions_many(ds, "tas", COMBOS, str(csv))
    for k in COMBOS:
        np.testing.assert_array_equal(got2[k].tas.values, got[k].tas.values)


def test_dataset_many_tas_poly_falls_back(torch_cuda):
    from climate_toolbox_amd import tas_poly, weighted_aggregate_grid_to_regions, weighted_aggregate_grid_to_regions_many
    ds, df = _ds_table(np.float32, False, T=30)
    tp = tas_poly(ds, 2, "tas-poly-2")
    got = weighted_aggregate_grid_to_regions_many(tp, "tas-poly-2", COMBOS, df)
    for (aggwt, agglev), out in got.items():
        ref = weighted_aggregate_grid_to_regions(tp, "tas-poly-2", aggwt, agglev, df)
        np.testing.assert_array_equal(np.asarray(out["tas-poly-2"].values), np.asarray(ref["tas-poly-2"].values))
