"""The apply entry layer from the outside, without a GPU: what the 30 exported wagg_*apply*_f32/_f64 symbols and wagg_apply()
answer when they refuse a call BEFORE any handle is dereferenced -- return code and wagg_last_error() text, compared exactly
with tests/golden/apply_entry_messages.json.

The file holds this library's own answers, recorded once from the commit before the typed entry layer (wagg_entry.h) became
templates on the element type (`python tests/test_apply_entry_host.py` rewrites it from the library that is built; do that
only on a commit whose texts are meant to become the reference).  It pins that every symbol still reaches wagg_apply with its
own element type ("f32" / "f64" in the message), plan kind, source and transform.

The cases are read off run_segment / run_dense (csrc/wagg_desc.hip): each is decided on the descriptor's fields alone, so the
plan handle 0x1000 (and the shard group 0x1000) is never looked at.  A case that would reach entry::is_many_plan(plan) or an
entry function is not here."""
import ctypes as C
import json
import os

import pytest

from climate_toolbox_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "apply_entry_messages.json")
FAKE = 0x1000
SYMBOLS = tuple(stem % t for stem in (
    "wagg_apply_%s", "wagg_apply_host_%s", "wagg_apply_host_ex_%s", "wagg_apply_host_multi_%s", "wagg_apply_poly_%s",
    "wagg_apply_poly_host_%s", "wagg_apply_edd_%s", "wagg_apply_edd_host_%s", "wagg_apply_sharded_%s", "wagg_dense_apply_%s",
    "wagg_dense_apply_poly_%s", "wagg_dense_apply_edd_%s", "wagg_dense_apply_host_%s", "wagg_dense_apply_host_multi_%s",
    "wagg_dense_apply_sharded_%s") for t in ("f32", "f64"))


def _null_call(L, name):
    """the symbol with a NULL plan (or plan array), zero sizes, NULL everywhere else"""
    fn = getattr(L, name)
    args = [0.0 if t is C.c_double else 0 if t in (C.c_int, C.c_int32, C.c_int64) else None for t in fn.argtypes]
    return fn(*args)


def _descriptor_cases():
    """(name, descriptor fields) of every refusal that is decided before a handle is dereferenced, for both element types"""
    TG, GT, TR, RT = _lib.LAYOUT_TG, _lib.LAYOUT_GT, _lib.OUT_TR, _lib.OUT_RT
    DEV, HOST, MULTI, SHARD = _lib.SRC_DEVICE, _lib.SRC_HOST, _lib.SRC_HOST_MULTI, _lib.SRC_SHARDED
    NONE, POLY, EDD = _lib.XF_NONE, _lib.XF_POLY, _lib.XF_EDD
    src = {DEV: "device", HOST: "host", MULTI: "multi", SHARD: "sharded"}
    xf = {NONE: "none", POLY: "poly", EDD: "edd"}
    extra = {DEV: {}, HOST: {}, MULTI: {"n_plans": 2}, SHARD: {"group": FAKE}}      # what wagg_apply itself asks of the source
    out = []
    for elem, en in ((_lib.T_F32, "f32"), (_lib.T_F64, "f64")):
        def add(name, kind, source, **f):
            d = dict(plan_kind=kind, elem=elem, source=source, plan=FAKE, transform=NONE, layout=TG, out_layout=TR)
            d.update(extra[source])
            d.update(f)
            out.append(("%s/%s/%s" % ("dense" if kind == _lib.PLAN_DENSE else "segment", en, name), d))
        D, S = _lib.PLAN_DENSE, _lib.PLAN_SEGMENT
        # dense-family plan
        for s in (DEV, HOST, MULTI, SHARD):
            add("layout-gt/" + src[s], D, s, layout=GT)
            add("out-rt/" + src[s], D, s, out_layout=RT)
            add("compact-rows/" + src[s], D, s, flags=_lib.APPLY_COMPACT_ROWS)
        for s in (MULTI, SHARD):
            add("exact-f32/" + src[s], D, s, flags=_lib.APPLY_EXACT_F32)
        for s in (HOST, MULTI, SHARD):
            for t in (POLY, EDD):
                add("transform-%s/%s" % (xf[t], src[s]), D, s, transform=t)
        for n_pow in (0, 2):
            add("poly-n_pow-%d" % n_pow, D, DEV, transform=POLY, n_pow=n_pow, pow_first=2)
        add("edd-n_thr-2", D, DEV, transform=EDD, n_thr=2, thresholds=FAKE)
        add("edd-n_thr-0", D, DEV, transform=EDD, n_thr=0, thresholds=FAKE)
        add("edd-thresholds-null", D, DEV, transform=EDD, n_thr=1)
        # segment-table plan
        CR = _lib.APPLY_COMPACT_ROWS
        for s in (HOST, MULTI, SHARD):
            add("compact-rows/source-" + src[s], S, s, flags=CR)
        for t in (POLY, EDD):
            add("compact-rows/transform-" + xf[t], S, DEV, flags=CR, transform=t)
        add("compact-rows/layout-gt", S, DEV, flags=CR, layout=GT)
        add("compact-rows/out-rt", S, DEV, flags=CR, out_layout=RT)
        for t in (POLY, EDD):
            add("host/transform-%s/layout-gt" % xf[t], S, HOST, transform=t, layout=GT)
            add("host/transform-%s/out-rt" % xf[t], S, HOST, transform=t, out_layout=RT)
        for s in (MULTI, SHARD):
            for t in (POLY, EDD):
                add("%s/transform-%s" % (src[s], xf[t]), S, s, transform=t)
            add(src[s] + "/layout-gt", S, s, layout=GT)
            add(src[s] + "/out-rt", S, s, out_layout=RT)
    return out


def _answers():
    """{case name: [return code, wagg_last_error() text]} from the library that is built"""
    L = _lib.load()
    got = {}
    for name in SYMBOLS:
        rc = _null_call(L, name)
        got["null-plan/" + name] = [rc, L.wagg_last_error().decode()]
    for name, fields in _descriptor_cases():
        d = _lib.ApplyDesc()
        d.struct_size = C.sizeof(d)
        d.pow_first = d.n_pow = 1
        for k, v in fields.items():
            setattr(d, k, v)
        rc = L.wagg_apply(C.byref(d))
        got[name] = [rc, L.wagg_last_error().decode()]
    return got


@pytest.fixture(scope="module")
def answers():
    return _answers()


def test_the_recorded_cases_are_the_cases_of_this_test(answers):
    golden = json.load(open(GOLDEN))
    assert len(SYMBOLS) == 30 and sorted(golden) == sorted(answers)


def test_every_refusal_is_a_status_with_a_message(answers):
    for name, (rc, text) in answers.items():
        assert rc in (-1, _lib.EUNSUPPORTED) and text, name
        if not name.startswith("null-plan/"):
            assert rc == _lib.EUNSUPPORTED and ("/ %s /" % name.split("/")[1]) in text, (name, text)


@pytest.mark.parametrize("prefix", ["null-plan/", "dense/f32/", "dense/f64/", "segment/f32/", "segment/f64/"])
def test_code_and_text_are_the_recorded_ones(answers, prefix):
    golden = json.load(open(GOLDEN))
    names = [n for n in golden if n.startswith(prefix)]
    assert names
    for name in names:
        assert answers[name] == golden[name], name


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump(_answers(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
