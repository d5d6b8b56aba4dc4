"""The scratch-memory catalogue (tests/scratch_catalogue.py) against the header, without a GPU: every entry include/aqg.h declares is
either run by a catalogue call or exempt with a reason, and the route / plan bits the calls expect cover every bit there is."""
import os
import re

import scratch_catalogue as cat
from aquery2_amd import capi as P
from test_cabi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_enum(prefix):
    src = open(os.path.join(ROOT, "include", "aqg.h")).read()
    return {m.group(1): int(m.group(2), 0) for m in re.finditer(r"\b(%s[A-Z0-9_]+)\s*=\s*(0x[0-9a-fA-F]+|\d+)" % prefix, src)}


def test_every_declared_entry_is_catalogued_or_exempt():
    declared = set(declared_symbols())
    exempt = set(cat.EXEMPT)
    assert all(cat.EXEMPT[n].strip() for n in exempt)
    assert not exempt - declared, ("exempt names the header does not declare", sorted(exempt - declared))
    named = set().union(*[set(c.entries) for c in cat.CALLS])
    assert not named & exempt, sorted(named & exempt)
    assert declared - exempt == named, {"not catalogued": sorted(declared - exempt - named), "not declared": sorted(named - declared)}


def test_names_are_unique_and_switch_sets_known():
    names = [c.name for c in cat.CALLS]
    assert len(names) == len(set(names))
    assert {c.switches for c in cat.CALLS} <= set(cat.SWITCH_SETS)
    # every switch set of tests/test_gpu_plans.py has a call of its own
    assert {c.switches for c in cat.CALLS} == set(cat.SWITCH_SETS)


def covered(kind):
    bits = 0
    for c in cat.CALLS:
        bits |= c.expect.get(kind, 0)
    return bits


def require(kind, enum):
    assert enum, kind
    missing = {n: v for n, v in enum.items() if not covered(kind) & v and (kind, v) not in cat.UNREACHABLE}
    assert not missing, (kind, missing)


def test_every_route_bit_is_expected_by_a_call():
    require("rank", header_enum("AQG_RANK_ROUTE_"))
    require("join", header_enum("AQG_JOIN_ROUTE_"))
    require("asof", header_enum("AQG_ASOF_ROUTE_"))
    require("str", header_enum("AQG_STR_ROUTE_"))
    assert ("str", P.STR_ROUTE_HOST) in cat.UNREACHABLE and set(cat.UNREACHABLE) == {("str", P.STR_ROUTE_HOST)}
    require("wj", {"STAGED": P.WJ_FOLD_STAGED, "INPLACE": P.WJ_FOLD_INPLACE})
    require("wj", {n: v for n, v in header_enum("AQG_ASOF_ROUTE_").items()})          # the window join's bounds take the as-of routes
    require("select", {"SMALL": P.ROUTE_SMALL, "GROUP": P.ROUTE_GROUP, "SPLIT": P.ROUTE_SPLIT})
    sort = set()
    for c in cat.CALLS:
        sort |= set(c.expect.get("sort", []))
    assert sort == {"%s:%d" % (path, k) for path in ("wg", "multi") for k in (0, 1, 2)}


def test_every_plan_bit_is_expected_by_a_call():
    plans = header_enum("AQG_PLAN_")
    assert len(plans) >= 17 and set(plans.values()) >= {getattr(P, n) for n in dir(P) if n.startswith("PLAN_")}
    require("plan", plans)
