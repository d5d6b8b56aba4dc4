"""include/aqg_pair.h without a GPU, as tests/test_cabi.py and tests/test_scratch_catalogue.py hold include/aqg.h: the library exports
every symbol the header declares, aqg.h includes the header, and every declared entry is run by a call of tests/pairwin_scratch.py or
exempt with a reason."""
import os
import re

import pairwin_scratch as ps
import scratch_catalogue as cat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "aqg_pair.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(aqg_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    import aquery2_amd
    lib = aquery2_amd.load_library()
    syms = declared_symbols()
    assert syms == ["aqg_grouped_scan2", "aqg_grouped_scan2_flat", "aqg_scan2", "aqg_scan2_last"]
    assert not [s for s in syms if not hasattr(lib, s)]
    assert '#include "aqg_pair.h"' in open(os.path.join(ROOT, "include", "aqg.h")).read()


def test_every_declared_entry_is_run_by_a_guard_call_or_exempt():
    declared, exempt = set(declared_symbols()), set(ps.EXEMPT)
    assert all(ps.EXEMPT[n].strip() for n in exempt) and not exempt - declared
    named = set().union(*[set(c.entries) for c in ps.CALLS])
    assert not named & exempt
    # (a call may also drive entries of aqg.h, which the catalogue holds: aqg_groupby_build)
    catalogued = set().union(*[set(c.entries) for c in cat.CALLS])
    assert declared - exempt == named - catalogued, {"not run": sorted(declared - exempt - named), "not declared": sorted(named - catalogued - declared)}
    assert len({c.name for c in ps.CALLS} | {c.name for c in cat.CALLS}) == len(ps.CALLS) + len(cat.CALLS)
    assert {c.family for c in ps.CALLS} == {ps.FAMILY} and ps.FAMILY not in {c.family for c in cat.CALLS}
