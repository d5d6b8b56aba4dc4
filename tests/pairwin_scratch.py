"""The scratch-memory calls of the pair windows: what tests/scratch_catalogue.py is for the entries of include/aqg.h, for those of
include/aqg_pair.h.  One small call per layout, each reaching REG, LDS and PREFIX, built from tests/pairwin_cases.py and checked by the
helper tests/test_gpu_pairwin.py uses.  Kept in a list of its own: tests/pairwin_scratch_child.py adds the calls to the catalogue inside
the child process it runs them in, tests/test_gpu_pairwin_guard.py holds them under the guard, tests/test_pairwin_cabi.py holds the list
to the header without a GPU."""
from scratch_catalogue import Call

EXEMPT = {"aqg_scan2_last": "reporter"}
FAMILY = "pairwin"
ALL_ROUTES = 1 | 2 | 4            # pairwin_cases.ROUTE_REG | ROUTE_LDS | ROUTE_PREFIX
CALLS = []


def call(name, entries):
    def deco(fn):
        CALLS.append(Call(name, entries, fn, family=FAMILY))
        return fn
    return deco


@call("pairwin_flat", ["aqg_scan2"])
def _pairwin_flat(env):
    import pairwin_cases as pc
    import test_gpu_pairwin as tp
    c = min((c for c in pc.flat_cases() if len(c.x) > pc.TS and c.long_ok), key=lambda c: len(c.x))
    assert tp.hold_case(env.dev, c) == ALL_ROUTES


@call("pairwin_grouped", ["aqg_grouped_scan2", "aqg_grouped_scan2_flat", "aqg_groupby_build"])
def _pairwin_grouped(env):
    import pairwin_cases as pc
    import test_gpu_pairwin as tp
    c = next(c for c in pc.grouped_cases() if c.name.startswith("grouped-halo3"))
    gb = env.dev.groupby_build([c.keys_row])
    assert tp.hold_case(env.dev, c, gb) == ALL_ROUTES
    return {"plan": gb.plan}
