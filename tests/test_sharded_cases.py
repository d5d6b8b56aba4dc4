"""tests/sharded_cases.py held to account, without a GPU: the cuts are what their names say, the inputs carry across shard borders where
they claim to, the models' right fold passes the comparisons the GPU tests apply -- and every corruption of that fold that the sharded layer
could suffer (sharded_cases.FAULTS) is refused by at least one (column, cut set) of the GPU test's own case list.  A corruption that
passed would mean that the inputs do not tell it apart.

Two of the corruptions need a word.  The reference seeds `max` with numeric_limits<T>::min() and `min` with ::max(), so in a REDUCTION the
type's own seed from a shard that does not hold the group (or holds no row) changes nothing: the oracle's max of a strictly negative
column is that seed already.  What such a shard can leak is (a) the zero-filled record it ships (`zero_moment_from_a_shard_without_rows`),
refused by an all-+Inf column's min and by one-row groups, and (b) the seed into an operation that has NONE -- minw / maxw with w == 0, the
running form (`type_seed_from_an_empty_shard`, and `running_min_from_the_seeded_moment`: the seeded min / max of the predecessors taken for their
true extreme), refused by the columns whose leading shards are strictly negative or all +Inf."""
import numpy as np
import pytest

import checker as ck
import extremes as ex
import groupagg_cases as gc
import sharded_cases as sc

FP32, FP64 = np.dtype(np.float32), np.dtype(np.float64)


def refused(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# ---- the cuts and the inputs ------------------------------------------------------------------------------------------------------------------
def test_cuts_are_what_they_are_named():
    for n in (sc.N, sc.N_TINY):
        names = sc.cut_names(n)
        assert set(names) >= {"even3", "tiny_middle", "empty_first", "empty_last", "empty_middle_then_tiny", "one_holds_all"}
        for c in names:
            sh = sc.shards(c, n)                                   # (asserts its own promises)
            assert 2 <= len(sh) <= 5 and sum(hi - lo for lo, hi in sh) == n
    assert {"tile_border", "tile_border_plus1"} <= set(sc.cut_names(sc.N)) and sc.BORDER % sc.TS == 0
    assert len(sc.shards("empty_middle_then_tiny", sc.N_TINY)) == 5 == sc.N_TINY           # as many ranks as rows, one of them empty
    even = sc.shards("even3", sc.N)
    assert max(hi - lo for lo, hi in even) < 25_000 < sc.N       # a 25 000-row window's halo spans two predecessors, and every shard is shorter than it
    assert all(w in sc.WINDOWS for w in (1, 2, 3, 5, 100, 128, 1000, 2500, 25_000, 50_000, sc.N, sc.N + 3))
    assert set(sc.RATIO_W) >= set(sc.gsc.RATIO_W) | {sc.N - 1, sc.N, sc.N + 5}
    assert set(sc.SCAN_OPS) == set(sc.gsc.OPS) - {"vars", "stddevs"}


def test_the_carry_happens_in_the_fold_across_shards():
    """every carry column under every cut with two shards that hold rows: two shard sums differ in their high word, or their low words add up past 2^64"""
    for dt in (sc.I64, sc.U64):
        for cname, x in sc.carry_columns(dt):
            for cut in sc.cut_names(sc.N):
                sums = [sc.exact_sum_fast(p) for p in sc.pieces(x, sc.shards(cut, sc.N)) if len(p)]
                if cut == "one_holds_all":
                    continue
                hi = {(s >> 64) & sc.M64 for s in sums}
                assert len(sums) >= 2 and (len(hi) >= 2 or sum(s & sc.M64 for s in sums) > sc.M64), (dt, cname, cut)


def test_the_probe_rows_lie_in_different_shards():
    for name, x, s in sc.probe_cases():
        assert sc.exact_sum_fast(x) == s
        cuts = sc.probe_cuts(len(x))
        tail = cuts["last-rows-apart"]
        assert [hi - lo for lo, hi in tail[1:]] == [1, 1, 1] or len(x) < 3
        assert cuts["one-row-last"][-1] == (len(x) - 1, len(x)) and cuts["one-row-last"][1][0] == cuts["one-row-last"][1][1]


# ---- the right fold passes ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole(oracle):
    """oracle.reduce of every reduce case's whole column, once"""
    return {c["name"]: {name: oracle.reduce(op, c["x"]) for name, op in ck.RED_NAMES.items()} for c in sc.reduce_cases()}


def reduce_model(oracle, case, sh, fault=None):
    return sc.fold_reduce(case["x"].dtype, [sc.shard_moments(oracle, p) for p in sc.pieces(case["x"], sh)], fault)


def check_reduce_model(case, got, want):
    for name in ck.RED_NAMES:
        sc.check_reduce(case, name, got[name], want[name], wv=want["var"], gv=got["var"])


def test_the_right_fold_of_the_moments_is_the_oracles_reduction(oracle, whole):
    for case in sc.reduce_cases():
        if case["kind"] == "nan":
            continue
        for cut in sc.cut_names(sc.N):
            check_reduce_model(case, reduce_model(oracle, case, sc.shards(cut, sc.N)), whole[case["name"]])
    for name, x, s in sc.probe_cases():
        case = dict(name=name, x=x, kind="int")
        want = {nm_: oracle.reduce(op, x) for nm_, op in ck.RED_NAMES.items()}
        assert want["sum"] == s and np.float64(want["avg"]).tobytes() == np.float64(float(s) / float(len(x))).tobytes()
        for sh in sc.probe_cuts(len(x)).values():
            check_reduce_model(case, reduce_model(oracle, case, sh), want)


MODEL_SCANS = [(np.int16, "sums", 0), (np.int64, "sums", 0), (np.uint64, "sums", 0), (np.int32, "mins", 0), (FP32, "maxs", 0), (FP64, "mins", 0), (np.int8, "minw", 0),
               (FP32, "maxw", 0), (FP64, "minw", 0), (np.uint16, "minw", 5), (np.int64, "maxw", 25_000), (FP32, "minw", sc.N + 3), (np.int32, "sumw", 100), (np.uint64, "sumw", 25_000),
               (FP64, "sumw", 5), (FP32, "avgw", 1000), (np.int16, "avgw", 2), (np.int64, "deltas", 0), (FP32, "prev", 0), (np.uint8, "aggnext", 0), (FP64, "aggnext", 0)] + \
              [(dt, "ratiow", w) for dt in (np.int32, FP64) for w in sc.RATIO_W]


def test_the_right_fold_of_the_scans_is_the_oracles_scan(oracle):
    """(the comparison without `sh`: "a window's rows are the window's" is a standard for the device's routes -- the oracle's recurrence, which the model
    is made of, has touched the whole prefix)"""
    for dt, name, w in MODEL_SCANS:
        for label, x in sc.scan_columns(np.dtype(dt).name, name):
            want = oracle.scan(ck.SCAN_NAMES[name], x, w)
            for cut in sc.cut_names(sc.N):
                sh = sc.shards(cut, sc.N)
                sc.check_scan(name, x, w, sc.model_scan(oracle, name, x, sh, w), want, what=f"{cut} {label}")
    for dt in (np.int16, FP32):                               # five rows over as many ranks
        for name in ("mins", "deltas", "prev", "aggnext", "minw", "maxw", "sumw", "ratiow"):
            for label, x in sc.scan_columns(np.dtype(dt).name, name, sc.N_TINY):
                for w in sc.windows_of(name, sc.N_TINY):
                    want = oracle.scan(ck.SCAN_NAMES[name], x, w)
                    for cut in sc.cut_names(sc.N_TINY):
                        sh = sc.shards(cut, sc.N_TINY)
                        sc.check_scan(name, x, w, sc.model_scan(oracle, name, x, sh, w), want, what=f"{cut} {label}")


# ---- every corruption is refused by a case of the GPU test's list -------------------------------------------------------------------------------
def reduce_refusal(oracle, whole, fault, kinds, cuts=None):
    for case in sc.reduce_cases():
        if case["kind"] not in kinds:
            continue
        for cut in cuts or sc.cut_names(sc.N):
            sh = sc.shards(cut, sc.N)
            if refused(lambda: check_reduce_model(case, reduce_model(oracle, case, sh, fault), whole[case["name"]])):
                return case["name"], cut
    return None


def scan_refusal(oracle, fault, names, dtypes=ex.NUM_DTYPES, cuts=None):
    for dt in dtypes:
        for name, label, x, w in sc.scan_plan(dt, sc.N, names):
            if name in ("minw", "maxw") and fault in ("type_seed_from_an_empty_shard", "running_min_from_the_seeded_moment") and w != 0:
                continue                                           # (these two are about the running form)
            want = oracle.scan(ck.SCAN_NAMES[name], x, w)
            for cut in cuts or sc.cut_names(sc.N):
                sh = sc.shards(cut, sc.N)
                if refused(lambda: sc.check_scan(name, x, w, sc.model_scan(oracle, name, x, sh, w, fault), want)):
                    return np.dtype(dt).name, name, label, w, cut
    return None


@pytest.mark.parametrize("fault", sc.FAULTS)
def test_a_corrupted_fold_is_refused(oracle, whole, fault):
    hit = None
    if fault in ("carry_high_word_dropped", "low_half_sign_extended"):
        hit = reduce_refusal(oracle, whole, fault, ("int",))
        assert hit and scan_refusal(oracle, fault, ("sums",), (sc.I64, sc.U64)), fault
    elif fault == "avg_rounded_per_shard":
        for name, x, s in sc.probe_cases():
            case, want = dict(name=name, x=x, kind="int"), {nm_: oracle.reduce(op, x) for nm_, op in ck.RED_NAMES.items()}
            for cname, sh in sc.probe_cuts(len(x)).items():
                if refused(lambda: check_reduce_model(case, reduce_model(oracle, case, sh, fault), want)):
                    hit = hit or (name, cname)
    elif fault == "var_n_plus_1_of_the_shard":
        hit = reduce_refusal(oracle, whole, fault, ("int",))
        assert hit and reduce_refusal(oracle, whole, fault, ("fp_sq",)), fault
    elif fault == "zero_moment_from_a_shard_without_rows":
        hit = reduce_refusal(oracle, whole, fault, ("fp_bits",))
        assert hit and groupby_refusal(oracle, fault), fault
    elif fault in ("type_seed_from_an_empty_shard", "running_min_from_the_seeded_moment"):
        hit = scan_refusal(oracle, fault, ("maxw",) if fault.startswith("type") else ("minw",), ex.FP_DTYPES)
        if fault.startswith("type"):
            assert hit and scan_refusal(oracle, fault, ("minw",), ex.FP_DTYPES), fault
    elif fault == "seed_from_the_predecessor_only":
        hit = scan_refusal(oracle, fault, ("mins", "maxs"), (np.int32, FP32), ("tiny_middle",))
    elif fault == "halo_of_the_nearest_shard_only":
        hit = scan_refusal(oracle, fault, ("sumw",), (np.int32,), ("tiny_middle",))
        for names, dts in ((("minw", "maxw"), (np.int16, FP64)), (("avgw",), (FP32,)), (("ratiow",), (np.int32,))):
            assert scan_refusal(oracle, fault, names, dts, ("tiny_middle", "even3")), (fault, names)
    elif fault == "next_from_an_empty_successor":
        hit = scan_refusal(oracle, fault, ("aggnext",), (np.int32, FP64), ("empty_middle_then_tiny",))
    elif fault == "ratiow_length_of_the_shard":
        hit = scan_refusal(oracle, fault, ("ratiow",), (np.int32, FP32))
    elif fault == "first_rows_local":
        hit = groupby_refusal(oracle, fault)
    assert hit, f"no case of the list refuses {fault}"
    print(f"{fault}: refused by {hit}")


# ---- the sharded group-by -----------------------------------------------------------------------------------------------------------------------
def test_the_group_by_cuts_put_the_groups_where_they_say(oracle):
    lay = sc.groupby_layout(300)
    cuts = sc.groupby_cuts(lay)
    assert set(cuts) == {"even3", "tiny_middle", "empty_rank", "split"} and any(hi == lo for lo, hi in cuts["empty_rank"])
    sh = cuts["split"]
    dominant = np.nonzero(lay.labels == 0)[0]
    assert len(dominant) == lay.n // 3 and sc.shards_holding(dominant, sh) == {1}                                  # (a)
    pinf, neg = sc.shards_holding(lay.sized_rows[0], sh), sc.shards_holding(lay.sized_rows[2], sh)                 # (b)
    assert len(pinf) == 1 and len(neg) == 1
    for r, (lo, hi) in enumerate(sh):
        assert len(np.unique(lay.labels[lo:hi])) > (1 if r != 1 else 0)
    assert all(len(np.unique(lay.labels[sh[r][0]:sh[r][1]])) > 50 for r in (0, 2))                                 # the other shards hold other groups
    x = gc.fp_inf(np.float64, lay, 1)
    assert np.all(np.isposinf(x[lay.sized_rows[0]])) and np.all(x[lay.sized_rows[2]] < 0)
    for dt in (sc.I64, sc.U64):                                                                                     # (c): every probe group lies in two shards or more
        cl = sc.groupby_carry_layout(300, dt.name)
        assert cl.probe_es == (53, 64) and len(cl.sized_rows) == 6
        csh = sc.groupby_cuts(cl)["split"]
        for rows in cl.sized_rows:
            assert len(rows) < 3 or len(sc.shards_holding(rows, csh)) >= 2, (dt, len(rows))
        assert sum(len(sc.shards_holding(rows, csh)) >= 2 for rows in cl.sized_rows) >= 3
    # most groups are missing from some shard of every cut, and the group count per shard fits the one-launch merge's 1024 / 3 rows
    for cname, sh in cuts.items():
        per = [len(np.unique(lay.labels[lo:hi])) for lo, hi in sh]
        assert max(per) <= sc.GMAX_SMALL and sc.GMAX_SMALL * len(sh) <= 1024, (cname, per)
    assert len(np.unique(lay.labels[cuts["tiny_middle"][1][0]:cuts["tiny_middle"][1][1]])) <= 3


GROUPBY_MODEL = [("int_full", np.int16, (gc.SUM, gc.MIN, gc.MAX, gc.COUNT, gc.AVG)), ("int_full", np.int64, (gc.SUM, gc.AVG, gc.MIN)), ("carry", np.uint64, (gc.SUM, gc.AVG)),
                 ("carry", np.int64, (gc.SUM, gc.AVG)), ("fp_inf", np.float32, (gc.MIN, gc.MAX)), ("fp_inf", np.float64, (gc.SUM, gc.MIN, gc.MAX))]


def groupby_model_cases():
    for setname, dt, ops in GROUPBY_MODEL:
        dt = np.dtype(dt)
        lay = sc.groupby_carry_layout(300, dt.name) if setname == "carry" else sc.groupby_layout(300)
        for cname, x, _ in gc.columns(lay, [dt], seed=300, sets=(setname,)):
            if "squares" not in cname:
                yield lay, cname, x, ops


def check_groupby_model(oracle, lay, x, ops, sh, fault=None):
    keys = gc.k_i32(lay.labels)
    o = oracle.groupby(keys)
    got = sc.model_groupby(oracle, keys, list(ops), [x] * len(ops), sh, fault)
    assert got["ngroups"] == o["ngroups"] and np.array_equal(got["first"], o["first_rows"].astype(np.int64))
    assert [k[0] for k in got["keys"]] == keys[0][o["first_rows"]].tolist()
    for j, op in enumerate(ops):
        gc.compare(op, x, got["res"][j], oracle.grouped_reduce(op, x, o), o, "model")


def groupby_refusal(oracle, fault):
    for lay, cname, x, ops in groupby_model_cases():
        for cut, sh in sc.groupby_cuts(lay).items():
            if refused(lambda: check_groupby_model(oracle, lay, x, ops, sh, fault)):
                return cname, cut
    return None


def test_the_right_merge_of_the_shard_tables_is_the_oracles_group_by(oracle):
    for lay, cname, x, ops in groupby_model_cases():
        for cut, sh in sc.groupby_cuts(lay).items():
            check_groupby_model(oracle, lay, x, ops, sh)
    for fault in ("carry_high_word_dropped", "low_half_sign_extended", "avg_rounded_per_shard"):
        assert groupby_refusal(oracle, fault), fault


def test_exchange_calls_fit_the_one_launch_merge():
    """the calls of the one-launch test: every op once, at most six payload columns, and -- by the condition of csrc/exchange.hip that takes_small_merge
    restates -- every call but the MIN / MAX of a floating column expected on xmerge_small_kernel; SUM, COUNT and AVG of both floating types among them"""
    for dt in gc.ALL_DT:
        for ops in ((gc.INT_OPS,) if dt.kind != "f" else (gc.FP_SUM_OPS, gc.FP_SQ_OPS)):
            calls = sc.pack_exchange_calls(ops, dt, minmax_apart=True)
            assert sorted(op for c in calls for op in c) == sorted(ops) and all(sc.payload_columns(c, dt) <= 6 for c in calls), dt
            small = [c for c in calls if sc.takes_small_merge(c, dt, 1, sc.GMAX_SMALL, 3)]
            assert [c for c in calls if c not in small] == ([[gc.MIN, gc.MAX]] if dt.kind == "f" and ops == gc.FP_SUM_OPS else []), (dt, calls)
            if dt.kind == "f":
                assert {op for c in small for op in c} == set(ops) - {gc.MIN, gc.MAX}
            assert not sc.takes_small_merge(sc.pack_exchange_calls(ops, dt, 8)[0], dt, 1, 0, 3) and not sc.takes_small_merge(calls[0], dt, 2, sc.GMAX_SMALL, 3)
            assert not sc.takes_small_merge(calls[0], dt, 1, 5200, 3)
    assert not sc.takes_small_merge(list(gc.FP_SUM_OPS), np.float64, 1, sc.GMAX_SMALL, 3)              # one floating MIN / MAX takes the whole call off the path
    assert sc.payload_columns([gc.VAR], np.int64) == 5 and sc.payload_columns([gc.VAR, gc.STDDEV, gc.AVG], np.int32) == 4 and sc.payload_columns([gc.SUM, gc.MIN], np.float64) == 2
