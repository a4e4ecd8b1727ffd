"""The argument checks of the four spell units (csrc/wagg_spell.h: wagg_spell_reduce_*, wagg_spell_span_*, wagg_cell_spells_*,
wagg_row_cell_spells_*), which share one host layer, and of the Python calls above them: every requirement alone says what it has
always said, to the letter, and calls that violate two at once report the one that has always come first.  Every check runs
before any device work, so none of this needs a GPU; the expected texts were recorded from the four separate host functions and
the per-function Python blocks that preceded the shared ones."""
import ctypes as C

import numpy as np
import pytest

P_ = C.c_void_p(0x1000)          # a device pointer no one may read
NAN, INF = float("nan"), float("inf")
DAYS, EVENTS, LONGEST, AMOUNT, EXCESS = range(5)


def _dbl(*v):
    return (C.c_double * len(v))(*v)


GOOD = dict(X=P_, T=10, n=8, ldx=8, rb=P_, rows=P_, P=2, n_rows=10, doy=P_, win=P_, offset=0.0, n_thr=5, L_=3, stat=DAYS, below=0, flags=0,
            out=P_, ldo=8, pstride=16, status=P_, work=None, work_bytes=0)


def _scalar(name):
    def call(L, suffix, thr=_dbl(30.0, 35.0, 25.0, 35.0, 40.0), **kw):
        a = dict(GOOD, **kw)
        return getattr(L, name + suffix)(
            a["X"], a["T"], a["n"], a["ldx"], a["rb"], a["rows"], a["P"], a["n_rows"], a["doy"], a["win"], a["offset"], thr, a["n_thr"],
            a["L_"], a["stat"], a["below"], a["flags"], a["out"], a["ldo"], a["pstride"], a["status"], a["work"], a["work_bytes"], None)
    return call


def _cell(name):
    def call(L, suffix, thr=P_, ldt=8, kstride=16, pmap=P_, M=2, **kw):
        a = dict(GOOD, **kw)
        return getattr(L, name + suffix)(
            a["X"], a["T"], a["n"], a["ldx"], a["rb"], a["rows"], a["P"], a["n_rows"], a["doy"], a["win"], a["offset"], thr, a["n_thr"], ldt,
            kstride, pmap, M, a["L_"], a["stat"], a["below"], a["flags"], a["out"], a["ldo"], a["pstride"], a["status"], a["work"],
            a["work_bytes"], None)
    return call


SIZES = "negative size (T=10, n=8, P=-1, n_rows=10)"
PAIRING = "doy_dev and win_dev go together: both given, or both NULL (no season)"
LAYOUT = "ldx / ldo smaller than n (ldx=8, ldo=7, n=8)"
MIN_LENGTH = "min_length must be 1..32767, got 0"
LONGEST_RULE = "WAGG_SPELL_LONGEST does not use min_length: it must be 1, got 2"
BELOW = "below must be 0 or 1, got 2"
# the family's own words: its flags message, its "stat must be" text, the greatest statistic it takes
SCALAR = ("unknown flags 0x40 (a spell count has no keep-NaN form)", "stat must be WAGG_SPELL_DAYS, _EVENTS or _LONGEST, got %d")
PER_CELL = ("unknown flags 0x40 (a per-cell spell count has no keep-NaN form)",
            "stat must be WAGG_SPELL_DAYS, _EVENTS, _LONGEST or WAGG_CELL_SPELL_AMOUNT, _EXCESS, got %d")
SUMS_RULE = "WAGG_CELL_SPELL_AMOUNT / _EXCESS have no run counter: min_length must be 1, got 2"
NO_MAP = {"wagg_cell_spells_": (dict(pmap=None, M=3, kstride=24), "plane_of_period_dev is NULL: allowed only for M == 1 or M == P (M=3, P=2)"),
          "wagg_row_cell_spells_": (dict(pmap=None), "plane_of_row_dev is NULL")}


def _said(L, call, suffix):
    def said(**kw):
        assert call(L, suffix, **kw) == -1, kw
        return L.wagg_last_error().decode()
    return said


def _shared(L, call, suffix, said, flags_msg, stat_msg):
    """what grouped_reduce and the tail of the spell checks say for all eight entry points"""
    # each requirement alone ...
    assert said(P=-1) == SIZES
    assert said(flags=64) == flags_msg
    assert said(n_thr=0) == "n_thr must be 1..64, got 0" and said(n_thr=65) == "n_thr must be 1..64, got 65"
    assert said(offset=NAN) == "offset must be finite" and said(offset=-INF) == "offset must be finite"
    assert said(L_=0) == MIN_LENGTH and said(L_=32768) == "min_length must be 1..32767, got 32768"
    assert said(stat=17, L_=1) == stat_msg % 17 and said(stat=-1) == stat_msg % -1
    assert said(stat=LONGEST, L_=2) == LONGEST_RULE
    assert said(below=2) == BELOW and said(below=-1) == "below must be 0 or 1, got -1"
    assert said(win=None) == PAIRING and said(doy=None) == PAIRING
    assert said(ldo=7) == LAYOUT
    assert said(pstride=15) == "out_pstride smaller than P * ldo"
    assert said(out=None) == "NULL pointer (out_dev)"
    assert said(X=None) == "NULL pointer (X_dev)"
    # ... and of two violated at once the earlier one speaks: sizes, flags, the family's list (min_length, stat, the rules of
    # single statistics and `below` are its tail), the doy / win pairing, the layout, and behind the empty return out and X.
    # (a bad stat cannot meet the LONGEST rule or the sums' rule in one call, nor the two rules each other: their places are
    # pinned through their neighbours)
    assert said(P=-1, flags=64) == SIZES
    assert said(flags=64, n_thr=0) == flags_msg and said(flags=64, below=2) == flags_msg
    assert said(n_thr=0, offset=NAN) == "n_thr must be 1..64, got 0"
    assert said(offset=NAN, L_=0) == "offset must be finite"
    assert said(L_=0, stat=17) == MIN_LENGTH and said(L_=0, stat=LONGEST) == MIN_LENGTH
    assert said(stat=17, below=2) == stat_msg % 17
    assert said(stat=LONGEST, L_=2, below=2) == LONGEST_RULE
    assert said(below=2, win=None) == BELOW and said(below=2, doy=None) == BELOW
    assert said(win=None, ldo=7) == PAIRING and said(doy=None, pstride=15) == PAIRING
    assert said(ldo=7, out=None) == LAYOUT and said(ldo=7, pstride=15) == LAYOUT
    assert said(pstride=15, status=None) == "out_pstride smaller than P * ldo"
    assert said(status=None, out=None) == "NULL pointer (status_dev / row_begin)"
    assert said(rows=None, out=None) == "NULL pointer (rows)"
    assert said(out=None, X=None) == "NULL pointer (out_dev)"
    # an empty call returns ahead of the out / field checks, but not ahead of the layout -- nor of the family's list
    assert call(L, suffix, P=0, out=None, X=None) == 0
    assert said(P=0, ldo=7, out=None) == LAYOUT
    assert said(P=0, below=2, out=None) == BELOW


@pytest.mark.parametrize("suffix", ["f32", "f64"])
@pytest.mark.parametrize("name", ["wagg_spell_reduce_", "wagg_spell_span_"])
def test_scalar_thresholds_the_first_violated_requirement_is_reported(name, suffix):
    from climate_toolbox_amd import _lib
    L = _lib.load()
    call = _scalar(name)
    said = _said(L, call, suffix)
    flags_msg, stat_msg = SCALAR
    _shared(L, call, suffix, said, flags_msg, stat_msg)
    nan1, inf1 = _dbl(30.0, NAN, 25.0, NAN, 40.0), _dbl(30.0, 35.0, -INF, 35.0, 40.0)
    assert said(thr=None) == "thresholds is NULL"
    assert said(thr=nan1) == "threshold 1 is NaN"
    assert said(thr=inf1) == "threshold 2 is infinite (a constant plane)"
    assert said(thr=_dbl(30.0, INF, 25.0, NAN, 40.0)) == "threshold 1 is infinite (a constant plane)"      # (threshold by threshold)
    assert call(L, suffix, thr=nan1, n_thr=1, P=0) == 0                    # only the first n_thr are looked at
    for stat in (AMOUNT, EXCESS):                                          # the two sums are the per-cell families' alone
        assert said(stat=stat, L_=1) == stat_msg % stat
    assert said(n_thr=0, thr=None) == "n_thr must be 1..64, got 0"
    assert said(thr=None, offset=NAN) == "thresholds is NULL"
    assert said(offset=INF, thr=nan1) == "offset must be finite"
    assert said(thr=nan1, L_=0) == "threshold 1 is NaN" and said(thr=inf1, L_=0) == "threshold 2 is infinite (a constant plane)"
    assert said(flags=64, thr=nan1) == flags_msg
    assert said(thr=nan1, win=None) == "threshold 1 is NaN"


@pytest.mark.parametrize("suffix", ["f32", "f64"])
@pytest.mark.parametrize("name", ["wagg_cell_spells_", "wagg_row_cell_spells_"])
def test_per_cell_thresholds_the_first_violated_requirement_is_reported(name, suffix):
    from climate_toolbox_amd import _lib
    L = _lib.load()
    call = _cell(name)
    said = _said(L, call, suffix)
    flags_msg, stat_msg = PER_CELL
    no_map, no_map_msg = NO_MAP[name]
    _shared(L, call, suffix, said, flags_msg, stat_msg)
    kstride_msg = "thr_kstride smaller than M * ldt"
    assert said(M=0) == "M must be at least 1, got 0" and said(M=-1) == "M must be at least 1, got -1"
    assert said(thr=None) == "thr_dev is NULL"
    assert said(ldt=7) == "ldt smaller than n (ldt=7, n=8)"
    assert said(kstride=15) == kstride_msg and said(M=3, kstride=23) == kstride_msg and said(ldt=2 ** 62, kstride=2 ** 62) == kstride_msg
    assert said(**no_map) == no_map_msg
    for stat in (AMOUNT, EXCESS):
        assert said(stat=stat, L_=2) == SUMS_RULE and call(L, suffix, stat=stat, L_=1, P=0) == 0
    assert said(n_thr=0, thr=None) == "n_thr must be 1..64, got 0" and said(n_thr=0, M=0) == "n_thr must be 1..64, got 0"
    assert said(M=0, thr=None) == "M must be at least 1, got 0"
    assert said(thr=None, ldt=7) == "thr_dev is NULL"
    assert said(ldt=7, kstride=15) == "ldt smaller than n (ldt=7, n=8)"
    assert said(kstride=15, pmap=None) == kstride_msg
    assert said(offset=NAN, **no_map) == no_map_msg
    assert said(L_=0, **no_map) == no_map_msg
    assert said(stat=AMOUNT, L_=0) == MIN_LENGTH
    assert said(stat=EXCESS, L_=2, below=2) == SUMS_RULE and said(stat=AMOUNT, L_=2, win=None) == SUMS_RULE
    assert said(flags=64, **no_map) == flags_msg
    assert said(win=None, **no_map) == no_map_msg
    if name == "wagg_cell_spells_":                                        # a NULL map: one plane, or one plane per period
        assert call(L, suffix, pmap=None, M=1, P=0) == 0 and call(L, suffix, pmap=None, M=2, n=0, ldx=0, ldo=0, ldt=0, kstride=0) == 0
        assert said(pmap=None, M=3, kstride=24, P=4, pstride=32) == \
            "plane_of_period_dev is NULL: allowed only for M == 1 or M == P (M=3, P=4)"
    else:
        assert said(pmap=None, M=1, P=0) == no_map_msg


# ---- the Python calls above them ---------------------------------------------------------------------------------------------------
SIDE = "side must be 'above' or 'below', got 'over'"
STAT3 = "stat must be 'days', 'events' or 'longest', got 'mean'"
STAT5 = "stat must be 'days', 'events', 'longest', 'amount' or 'excess', got 'mean'"
# engine level: (arguments, text), in the order of the checks
ENGINE = [(dict(side="over"), SIDE),
          (dict(min_length=0), "min_length must be an integer in 1..32767, got 0"),
          (dict(min_length=32768), "min_length must be an integer in 1..32767, got 32768"),
          (dict(min_length=True), "min_length must be an integer in 1..32767, got True"),
          (dict(min_length=2.0), "min_length must be an integer in 1..32767, got 2.0"),
          (dict(min_length=None), "min_length must be an integer in 1..32767, got None"),
          (dict(stat="longest", min_length=2), "stat='longest' does not use min_length: it must be 1, got 2"),
          (dict(side="over", min_length=0), SIDE),
          (dict(stat="longest", min_length=0), "min_length must be an integer in 1..32767, got 0")]


class _NoTensor:
    """stands where engine.spell_reduce wants its field: the checks under test touch no tensor"""


def test_engine_spell_reduce_texts(monkeypatch):
    """engine.spell_reduce checks X first, which needs a CUDA tensor: with that one check stepped over, the rest raises before
    any device work"""
    from climate_toolbox_amd import engine
    monkeypatch.setattr(engine, "_check_X", lambda X, dims: X)
    for span in ("period", "record"):
        for kw, text in [(dict(stat="mean"), STAT3), (dict(stat="amount"), STAT3.replace("'mean'", "'amount'")),
                         (dict(stat="mean", side="over"), STAT3)] + ENGINE:
            with pytest.raises(ValueError) as e:
                engine.spell_reduce(_NoTensor(), [0, 1], [0], 0.0, [30.0], span=span, **kw)
            assert str(e.value) == text, kw
    with pytest.raises(ValueError) as e:
        engine.spell_reduce(_NoTensor(), [0, 1], [0], 0.0, [30.0, NAN], stat="mean")
    assert str(e.value) == "thresholds must be finite, got [30.0, nan]"                   # (the thresholds come first)


def test_engine_helper_texts():
    """the helper behind engine.spell_reduce and relative.cell_spell_reduce, for both tables of statistics; the sums' min_length
    rule is the per-cell call's own and comes behind it"""
    from climate_toolbox_amd import _lib, engine, relative
    for table, stat_text in ((engine._SPELL_STATS, STAT3), (relative._STATS, STAT5)):
        for kw, text in [(dict(stat="mean"), stat_text), (dict(stat="mean", side="over"), stat_text)] + ENGINE:
            a = dict(dict(stat="days", side="above", min_length=1), **kw)
            with pytest.raises(ValueError) as e:
                engine._spell_codes(table, a["stat"], a["side"], a["min_length"])
            assert str(e.value) == text, kw
    assert engine._spell_codes(engine._SPELL_STATS, "events", "below", np.int64(4)) == (4, _lib.SPELL_EVENTS, 1)
    assert engine._spell_codes(relative._STATS, "excess", "above", 1) == (1, _lib.CELL_SPELL_EXCESS, 0)
    assert engine._spell_codes(relative._STATS, "longest", "above", 1) == (1, _lib.SPELL_LONGEST, 0)
    with pytest.raises(ValueError) as e:
        engine._spell_codes(engine._SPELL_STATS, "amount", "above", 1)
    assert str(e.value) == STAT3.replace("'mean'", "'amount'")


PUBLIC = [(dict(side="over"), SIDE),
          (dict(min_length=0), "min_length must be an integer in 1..32767, got 0"),
          (dict(min_length=32768), "min_length must be an integer in 1..32767, got 32768"),
          (dict(min_length=True), "min_length must be an integer in 1..32767, got True"),
          (dict(min_length="3"), "min_length must be an integer in 1..32767, got '3'"),
          (dict(stat="longest", min_length=2), "stat='longest' does not use min_length (leave it out, or pass 1), got 2"),
          (dict(stat="longest", min_length=32767), "stat='longest' does not use min_length (leave it out, or pass 1), got 32767"),
          (dict(side="over", min_length=0), SIDE),
          (dict(stat="longest", min_length=0), "min_length must be an integer in 1..32767, got 0")]


def test_tas_spell_aggregate_texts():
    from climate_toolbox_amd import tas_spell_aggregate
    call = lambda **kw: tas_spell_aggregate(None, [35.0, 30.0], "popwt", "hierid", {}, **kw)
    for kw, text in [(dict(stat="mean"), STAT3), (dict(stat="excess"), STAT3.replace("'mean'", "'excess'")),
                     (dict(stat="mean", side="over"), STAT3)] + PUBLIC:
        with pytest.raises(ValueError) as e:
            call(**kw)
        assert str(e.value) == text, kw
    with pytest.raises(ValueError) as e:
        call(span="year", stat="mean")
    assert str(e.value) == "span must be 'period' or 'record', got 'year'"                # (span comes before stat)
    for fine in ({}, dict(stat="longest"), dict(stat="longest", min_length=1), dict(stat="longest", min_length=3), dict(min_length=32767)):
        with pytest.raises(ValueError, match="needs period="):           # the default counts as unset: the next check is reached
            call(period=None, **fine)


def test_tas_relative_spell_aggregate_texts():
    from climate_toolbox_amd import tas_relative_spell_aggregate
    from climate_toolbox_amd.relative import CellThresholds
    grid = (np.array([0.0, 0.5]), np.arange(4) * 0.5)
    th = CellThresholds.from_array(np.zeros((2, 4)), *grid)
    call = lambda **kw: tas_relative_spell_aggregate(None, kw.pop("th", th), "popwt", "hierid", {}, **kw)
    with pytest.raises(TypeError) as e:
        call(th=[30.0], stat="mean")
    assert str(e.value) == "thresholds must be a CellThresholds (relative.cell_quantiles or CellThresholds.from_array), got 'list'"
    sums = [(dict(stat=s, min_length=m), "stat=%r does not use min_length (leave it out, or pass 1), got %d" % (s, m))
            for s in ("amount", "excess") for m in (2, 6)]
    for kw, text in [(dict(stat="mean"), STAT5), (dict(stat="mean", side="over"), STAT5)] + PUBLIC + sums:
        with pytest.raises(ValueError) as e:
            call(**kw)
        assert str(e.value) == text, kw
    shifted = CellThresholds.from_array(np.zeros((2, 4)), *grid, shift=-273.15)
    amount = ("stat='amount' needs thresholds in final units (thresholds.shift == 0, got -273.15): one offset serves the comparison and "
              "the sum, so the amount against shifted thresholds would be a sum of raw values; stat='excess' has no such limit")
    for kw in (dict(), dict(min_length=1), dict(period=None)):
        with pytest.raises(ValueError) as e:
            call(th=shifted, stat="amount", **kw)
        assert str(e.value) == amount, kw
    with pytest.raises(ValueError) as e:                                  # min_length, then planes, then the amount's rule
        call(th=shifted, stat="amount", min_length=2, planes="year")
    assert str(e.value) == "stat='amount' does not use min_length (leave it out, or pass 1), got 2"
    with pytest.raises(ValueError) as e:
        call(th=shifted, stat="amount", planes="year")
    assert str(e.value) == "planes must be None, 'month', 'calendar_day' or a callable, got 'year'"
    for fine in (dict(th=shifted, stat="excess"), dict(stat="amount"), dict(stat="amount", min_length=3), dict(stat="longest", min_length=1)):
        with pytest.raises(ValueError, match="needs period="):
            call(period=None, **fine)
