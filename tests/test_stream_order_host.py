"""Completeness guard for tests/test_gpu_stream_order.py (no GPU): every public function and method of
climate_toolbox_amd.engine whose signature has a ``stream`` parameter is a key of that module's PROBES table, or is in its EXEMPT
dict with a one-line reason -- so a new ``stream=`` entry point cannot arrive without a probe.  (Private helpers -- names with a
leading underscore -- are reached through the public calls that hand their ``stream`` down.)"""
import inspect

from climate_toolbox_amd import engine
from tests import test_gpu_stream_order as probes


def _stream_entry_points():
    found = {}
    for name, obj in vars(engine).items():
        if name.startswith("_") or getattr(obj, "__module__", None) != engine.__name__:
            continue
        if inspect.isfunction(obj):
            members = [(name, obj)]
        elif inspect.isclass(obj):
            members = [("%s.%s" % (name, m), f) for m, f in vars(obj).items() if not m.startswith("_")
                       for f in [f.__func__ if isinstance(f, (staticmethod, classmethod)) else f] if inspect.isfunction(f)]
        else:
            continue
        for qual, f in members:
            if "stream" in inspect.signature(f).parameters:
                found[qual] = f
    return found


def test_every_stream_entry_point_is_probed_or_exempt():
    found = _stream_entry_points()
    assert len(found) >= 30 and "period_reduce" in found and "quantile_select" in found and "SparsePlan.apply" in found and "DensePlan.saw_inf" in found, sorted(found)
    missing = sorted(set(found) - set(probes.PROBES) - set(probes.EXEMPT))
    assert not missing, "engine entry points with stream= that tests/test_gpu_stream_order.py neither probes nor exempts: %s" % missing
    gone = sorted((set(probes.PROBES) | set(probes.EXEMPT)) - set(found))
    assert not gone, "PROBES / EXEMPT name what engine no longer has (or what no longer takes stream=): %s" % gone


def test_exempt_and_blocking_are_closed_lists():
    """EXEMPT: profile_event_overhead (it returns no data) and what the safety rule keeps out of probe B (take_axis: it uploads
    its index), each with a reason; an entry that is exempt from probe B only still has its probe A.  BLOCKING: the calls whose
    docstring says that they synchronise, with the sentence that says so."""
    assert set(probes.EXEMPT) == {"profile_event_overhead", "take_axis"}
    assert all(isinstance(r, str) and r.strip() and "\n" not in r for r in probes.EXEMPT.values())
    assert "take_axis" in probes.PROBES and "profile_event_overhead" not in probes.PROBES
    found = _stream_entry_points()
    for name, sentence in probes.BLOCKING.items():
        if name in found:
            doc = " ".join((found[name].__doc__ or "").split())
            assert sentence in doc, "%s: its docstring no longer says %r" % (name, sentence)
        else:
            assert name == "row lists given as host integers"
            assert sentence in " ".join(engine.period_reduce.__doc__.split())


def test_every_probe_names_its_element_types():
    for name, (dtypes, build) in probes.PROBES.items():
        assert dtypes and set(dtypes) <= {probes.F32, probes.F64} and callable(build), name
    both = [n for n, (d, _) in probes.PROBES.items() if len(d) == 2]
    assert sorted(set(probes.PROBES) - set(both)) == ["season_mask"]          # (its result is float64 whatever comes in)
