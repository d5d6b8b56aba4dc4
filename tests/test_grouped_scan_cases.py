"""tests/grouped_scan_cases.py held to account, without a GPU: the windows land on the routes they are named for, the layouts put
group starts where they say (against the oracle's group-by), the vector forms of the per-group comparisons decide as the per-group
calls do -- and the comparison the GPU tests apply refuses the oracle's own composition once it is corrupted in the ways the per-group
kernels could be wrong (a corruption that passed would mean that the inputs do not tell it apart)."""
import numpy as np
import pytest

import checker as ck
import exact_moments as em
import extremes as ex
import grouped_scan_cases as gc
from test_gpu_extremes import check_fp_sums, check_int_avgw
from test_gpu_grouped_scan import compose, flat_groups, pos_in_group

MUT_DTYPES = [np.dtype(t) for t in (np.int16, np.int64, np.uint64, np.float32, np.float64)]


def test_routes_are_the_ones_named():
    assert (gc.TS, gc.HALO_MAX_BYTES, gc.DIRECT_MAX_W, gc.VAR_REG_W, gc.VAR_DIRECT_MAX_W) == (2048, 98304, 64, 8, 64)
    for lname in gc.LAYOUTS:
        n = gc.layout(lname).n
        for dt in ex.NUM_DTYPES:
            for fam, route_of in gc.ROUTE_OF.items():
                named = gc.windows(fam, dt, n)
                for route, w in named:
                    assert route_of(dt, n, w) == route, (lname, dt, fam, route, w)
                want = {"sumwin": {"tile", "hbm"} | ({"direct"} if dt.kind == "f" else set()), "minmaxwin": {"registers", "lds", "hbm", "running"},
                        "variance": {"registers", "lds", "hbm"}}[fam]
                assert {r for r, _ in named} == want, (dt, fam)
    # the thresholds themselves (docstring of test_gpu_window_paths.py): the last window of the tile kernels and the first through HBM
    assert [gc.first_hbm_w(gc.minmax_route, np.dtype(t)) for t in (np.int8, np.int16, np.int32, np.int64)] == [22522, 14330, 7778, 3410]
    assert gc.first_hbm_w(gc.sum_route, np.int64) == 3906 and gc.first_hbm_w(gc.sum_route, np.int32) == gc.first_hbm_w(gc.sum_route, np.float64) == 9514
    for dt in ex.NUM_DTYPES:
        assert gc.minmax_route(dt, 1 << 30, gc.first_hbm_w(gc.minmax_route, dt) - 1) == "lds" and gc.sum_route(dt, 1 << 30, gc.first_hbm_w(gc.sum_route, dt) - 1) == "tile"
    assert gc.minmax_route(np.int8, 100, 100) == gc.minmax_route(np.int8, 100, 0) == "running" and gc.minmax_route(np.int8, 101, 100) == "lds"
    assert gc.minmax_route(np.int8, 1000, 15) == "registers" and gc.minmax_route(np.int8, 1000, 16) == "lds" and gc.minmax_route(np.int8, 1000, 2) == "registers"
    assert gc.sum_route(np.float32, 1000, 64) == "direct" and gc.sum_route(np.float32, 1000, 65) == "tile" and gc.sum_route(np.int32, 1000, 2) == "tile"
    assert [gc.var_route(np.int32, 1000, w) for w in (8, 9, 64, 65)] == ["registers", "lds", "lds", "hbm"]
    # the two-level carry scan: just above 4 * CH tiles, five chunks
    nt = (gc.TWO_LEVEL_N + gc.TS - 1) // gc.TS
    assert nt == gc.TWO_LEVEL_TILES + 2 and (nt + 2047) // 2048 == 5
    assert 4 * gc.CHUNK_ROWS in gc.TWO_LEVEL_STARTS and 4 * gc.CHUNK_ROWS - 1 in gc.TWO_LEVEL_STARTS and (nt - 1) * gc.TS in gc.TWO_LEVEL_STARTS
    assert len(gc.TWO_LEVEL_STARTS) == 5 and max(gc.TWO_LEVEL_STARTS) < gc.TWO_LEVEL_N


@pytest.mark.parametrize("lname", gc.LAYOUTS)
def test_layouts_put_the_starts_where_they_say(oracle, lname):
    lay = gc.layout(lname)
    ogb = oracle.groupby([lay.keys])
    assert ogb["ngroups"] == lay.G and np.array_equal(ogb["counts"], lay.sizes) and np.array_equal(ogb["offsets"], lay.offsets[:-1])
    assert np.array_equal(ogb["row_ids"], lay.row_ids)
    assert all(np.array_equal(ogb[k], lay.ogb[k]) for k in ("counts", "offsets", "row_ids"))
    assert np.array_equal(lay.pos, pos_in_group(ogb, lay.n)) and [(int(s), int(c)) for s, c in zip(lay.starts(), lay.sizes)] == flat_groups(ogb)
    flat = np.arange(lay.n)
    assert np.array_equal(lay.scatter(flat)[lay.row_ids], flat)
    assert 20_000 <= lay.n <= 60_000 and lay.n > gc.WIDEST_HBM_W            # every through-HBM window is shorter than the column: no running form instead
    starts, sizes = set(lay.starts().tolist()), lay.sizes.tolist()
    if lname == "borders":
        assert starts >= set(gc.BORDER_STARTS)
        assert any(sizes[i:i + 20] == [1] * 20 for i in range(lay.G)) and any(sizes[i:i + 20] == [2] * 20 for i in range(lay.G))
        for w in gc.BORDER_W:
            assert {w - 1, w, w + 1} - {0} <= set(sizes), w
        used = {w for dt in ex.NUM_DTYPES for fam in gc.ROUTE_OF for r, w in gc.windows(fam, dt, lay.n) if r in ("direct", "tile", "registers", "lds")}
        assert used | set(gc.RATIO_W) <= set(gc.BORDER_W)
        g = int(np.argmax(lay.sizes))
        assert sizes[g] > max(gc.BORDER_W) and lay.offsets[g + 1] // gc.TS - lay.offsets[g] // gc.TS >= 10
    if lname == "wide":
        long_ = [g for g in range(lay.G) if sizes[g] > gc.WIDEST_HBM_W]
        assert len(long_) == 2
        for g in long_:                                                  # the next group starts inside the reach of a window that ends in the group behind it
            assert sizes[g + 1] < 100 and lay.offsets[g + 2] - lay.offsets[g + 1] < min(gc.first_hbm_w(r, dt) for r in (gc.sum_route, gc.minmax_route) for dt in ex.NUM_DTYPES)
    if lname == "dense":
        assert set(sizes) == {1, 2, 3} and abs(lay.G / lay.n - 0.5) < 0.02
        per_block = np.bincount(lay.starts() // 8)
        assert per_block.min() >= 2                                      # every lane block of eight positions holds several starts


def test_group_accumulate_is_cumsum_per_group():
    for lname in gc.LAYOUTS:
        lay = gc.layout(lname)
        a = np.abs(ex.sum_safe(ex.unary_column(np.dtype(np.float64), lay.n, 12, nan=False, inf=False)))
        assert gc.group_accumulate(lay, a).tobytes() == gc.compose_flat(lay, a, np.cumsum, np.float64).tobytes()
        b = np.random.default_rng(13).random(lay.n) < 0.2
        assert np.array_equal(gc.group_accumulate(lay, b, np.maximum), gc.compose_flat(lay, b, np.maximum.accumulate, bool))


def test_expected_is_the_composition_of_the_existing_tests(oracle):
    for lname, dt, name, w in (("borders", np.int64, "sums", 0), ("borders", np.float32, "ratiow", 7), ("dense", np.uint8, "minw", 3), ("wide", np.float64, "avgw", 100),
                               ("borders", np.int16, "aggnext", 0)):
        lay = gc.layout(lname)
        flat = ex.unary_column(np.dtype(dt), lay.n, 11, nan=False, inf=False)
        op = ck.SCAN_NAMES[name]
        want = compose(oracle.groupby([lay.keys]), lay.scatter(flat), lambda v: oracle.scan(op, v, w), gc.out_dtype(oracle, name, flat.dtype))
        assert ex.same(gc.expected(oracle, lay, name, flat, w), want), (lname, name)
        assert ex.same(gc.compose_flat(lay, flat, lambda v: oracle.scan(op, v, w), want.dtype), want), (lname, name)
        across = gc.compose_flat(lay, flat, lambda v: oracle.scan(op, v, w), want.dtype, left=1, right=1)        # the corruptions' form
        assert ex.same(gc.expected(oracle, lay, name, flat, w, left=1, right=1), across) and not ex.same(across, want), (lname, name)


@pytest.mark.parametrize("lname", ["borders", "dense"])
def test_vector_forms_are_the_per_group_calls(oracle, lname):
    """fp_sums_bad / int_avgw_bad against check_fp_sums / check_int_avgw called on every group's slice, on results pushed off the oracle's by
    zero to two bounds: the same groups are refused"""
    lay = gc.layout(lname)
    rng = np.random.default_rng(5)
    groups = flat_groups(lay.ogb)

    def refused_per_group(fn):
        out = set()
        for g, (s, c) in enumerate(groups):
            try:
                fn(slice(s, s + c))
            except AssertionError:
                out.add(g)
        return out

    full = lname == "borders"                                            # ("dense": twelve thousand calls per loop -- two columns, two ops, one type)
    for dt in ex.FP_DTYPES if full else ex.FP_DTYPES[:1]:
        for cname, flat in gc.columns(lay, dt, "sumwin", "sumw")[::1 if full else 2]:
            for name, w in (("sums", 0), ("avgs", 0), ("sumw", 5), ("avgw", 100)) if full else (("avgs", 0), ("sumw", 5)):
                want = gc.expected(oracle, lay, name, flat, w)
                _, _, _, _, bound = gc.fp_sums_bad(name, want, want, flat, lay, w)
                with np.errstate(invalid="ignore"):
                    got = want + rng.choice([0.0, 0.5, 2.0, -2.0], lay.n, p=[0.9, 0.04, 0.03, 0.03]) * bound
                    got[rng.random(lay.n) < 0.01] = np.nan
                bad = gc.fp_sums_bad(name, got, want, flat, lay, w)[0]
                loop = refused_per_group(lambda r: check_fp_sums(name, got[r], want[r], flat[r], w if w else None))
                assert set(lay.gid[bad].tolist()) == loop and (loop or cname != "finite"), (lname, dt, cname, name)
    for dt in (np.dtype(np.int8), np.dtype(np.int64)) if full else (np.dtype(np.int64),):
        flat = gc.columns(lay, dt, "sumwin", "avgw")[0][1]
        for w in (5, 100) if full else (2,):
            exact = gc.int_avgw_bad(np.zeros(lay.n), flat, lay, w)[1]
            got = exact + rng.choice([0, 1, 3, -3], lay.n, p=[0.9, 0.04, 0.03, 0.03]) * np.spacing(np.abs(exact))
            bad = gc.int_avgw_bad(got, flat, lay, w)[0]
            loop = refused_per_group(lambda r: check_int_avgw(got[r], flat[r], w))
            assert set(lay.gid[bad].tolist()) == loop and loop, (lname, dt, w)


# ---- the comparison refuses what the kernels could get wrong ------------------------------------------------------------------------------
def family_of(name):
    return next(f for f, ops in gc.FAMILIES.items() if name in ops)


def column_of(lay, dt, name):
    return gc.columns(lay, dt, family_of(name), name)[0][1]


def window_of(name, dt, lay, route=None):
    """a window of the op on an LDS route (the first one named, or the one on `route`)"""
    if name == "ratiow":
        return 7
    fam = family_of(name)
    if fam not in gc.ROUTE_OF or name in ("vars", "stddevs"):
        return 0
    return next(w for r, w in gc.windows(fam, dt, lay.n) if (r == route if route else r != "running"))


def refuses(name, lay, flat, w, got, want):
    try:
        gc.check(name, lay, flat, w, got, want, "corrupted")
    except AssertionError:
        return True
    return False


def some_column_refuses(oracle, name, lay, dt, w, corrupt):
    """the GPU test runs every column of gc.columns: a corruption has to be refused on one of them"""
    return any(refuses(name, lay, flat, w, corrupt(flat), gc.expected(oracle, lay, name, flat, w)) for _, flat in gc.columns(lay, dt, family_of(name), name))


def usable(name, dt):
    return not (name == "avgw" and dt.kind == "u" and dt.itemsize >= 4)


def truth(oracle, lay, name, flat, w):
    """a result the comparison has to ACCEPT: the oracle's composition; for the ops held to values computed here (variances, integer avgw,
    floating windows on the direct and tile routes) those values"""
    if name in gc.VAR_OPS:
        T = em.Exact(flat, lay.offsets).var(None if name in ("vars", "stddevs") else w)
        return np.sqrt(T) if name.startswith("stddev") else T
    if name == "avgw" and flat.dtype.kind != "f":
        return gc.int_avgw_bad(np.zeros(lay.n), flat, lay, w)[1]
    if name in ("sumw", "avgw") and flat.dtype.kind == "f":
        s = gc.trail_grouped(lay, flat.astype(np.float64), w)
        return s / np.minimum(lay.pos + 1, w) if name == "avgw" else s
    return gc.expected(oracle, lay, name, flat, w)


@pytest.mark.parametrize("dt", MUT_DTYPES, ids=ex.nm)
def test_the_comparison_accepts_a_right_answer(oracle, dt):
    lay = gc.layout("borders")
    for name in gc.OPS:
        if usable(name, dt):
            flat, w = column_of(lay, dt, name), window_of(name, dt, lay)
            gc.check(name, lay, flat, w, truth(oracle, lay, name, flat, w), gc.expected(oracle, lay, name, flat, w), "truth")


@pytest.mark.parametrize("dt", MUT_DTYPES, ids=ex.nm)
def test_no_reset_at_a_group_start_is_refused(oracle, dt):
    """the whole-column scan of the flat column in place of the per-group one"""
    for lname in ("borders", "dense"):
        lay = gc.layout(lname)
        for name in gc.OPS:
            if usable(name, dt):
                w = window_of(name, dt, lay)
                assert some_column_refuses(oracle, name, lay, dt, w, lambda flat: oracle.scan(ck.SCAN_NAMES[name], flat, w)), (lname, name, w)


@pytest.mark.parametrize("dt", MUT_DTYPES, ids=ex.nm)
def test_windows_and_shifts_across_a_border_are_refused(oracle, dt):
    """a window that reaches one row across a start; a window clamped one row early; aggnext reading across a group's end; prev and deltas
    reading across a start"""
    lays = [gc.layout("borders"), gc.layout("wide")]              # ("wide": the groups longer than the windows that go through HBM)
    lay = lays[0]
    some_refuses = lambda name, w, corrupt: any(some_column_refuses(oracle, name, l, dt, w, lambda flat: corrupt(l, flat)) for l in lays)
    for name in ("sumw", "avgw", "minw", "maxw", "varw", "stddevw", "ratiow"):
        if not usable(name, dt):
            continue
        routes = [None] if name == "ratiow" else [r for r, _ in gc.windows(family_of(name), dt, lay.n) if r != "running"]
        for route in routes:
            w = window_of(name, dt, lay, route)
            assert some_refuses(name, w, lambda l, flat: gc.expected(oracle, l, name, flat, w, left=1)), (name, w, "one row across a start")
            if name != "ratiow":
                assert some_refuses(name, w, lambda l, flat: gc.expected(oracle, l, name, flat, w - 1)), (name, w, "clamped one row early")
    for name, kw in (("aggnext", dict(right=1)), ("prev", dict(left=1)), ("deltas", dict(left=1))):
        for lname in ("borders", "dense"):
            lay = gc.layout(lname)
            assert some_column_refuses(oracle, name, lay, dt, 0, lambda flat: gc.expected(oracle, lay, name, flat, 0, **kw)), (lname, name)


@pytest.mark.parametrize("dt", [np.dtype(np.int64), np.dtype(np.uint64)], ids=ex.nm)
def test_avgs_without_the_first_rows_rounding_is_refused(oracle, dt):
    """float(exact sum of the group so far) / rows in place of the reference's sum that starts from the first row as a double: for every
    planted first row it differs in EVERY one of the named groups -- on the second row, on the last row of the quiet stretch and, for
    the groups that reach into the next tile, on rows there"""
    lay = gc.layout("first-rows")
    for first, flat in gc.planted_first_rows(lay, dt):
        want = gc.expected(oracle, lay, "avgs", flat)
        exact = gc.compose_flat(lay, flat.astype(object), np.cumsum, object).astype(np.float64) / (lay.pos + 1)
        differs = ~np.array([ex.same(exact[i:i + 1], want[i:i + 1]) for i in range(lay.n)])
        for start in gc.FIRST_ROW_STARTS:
            rows = gc.planted_rows(lay, start)
            c = int(rows.sum()) + 1
            quiet = min(c, gc.QUIET_ROWS)
            assert gc.same_rows(exact, want, rows) == start + 1 and differs[start + quiet - 1], (int(first), start)
            if start // gc.TS != (start + quiet - 1) // gc.TS:                      # the group goes on into the next tile: rows there tell as well
                nxt = (start // gc.TS + 1) * gc.TS
                assert differs[nxt:start + quiet].sum() >= (start + quiet - nxt) // 2, (int(first), start)
            assert gc.same_rows(want, want, rows) < 0
        assert refuses("avgs", lay, flat, 0, exact, want), int(first)


def test_first_row_layout_puts_long_groups_on_the_named_starts(oracle):
    lay = gc.layout("first-rows")
    ogb = oracle.groupby([lay.keys])
    assert np.array_equal(ogb["counts"], lay.sizes) and np.array_equal(ogb["offsets"], lay.offsets[:-1]) and np.array_equal(ogb["row_ids"], lay.row_ids)
    st = gc.FIRST_ROW_STARTS
    assert set(st) <= set(lay.starts().tolist()) and all(lay.sizes[lay.group_at(p)] >= 8 for p in st)
    assert sum(p % gc.TS == 0 for p in st) >= 3 and any(p % gc.TS == 0 and p for p in st)           # tile borders, not only position 0
    assert any(p % gc.TS == gc.TS - 1 and lay.sizes[lay.group_at(p)] > gc.TS for p in st)           # a tile's last position; the group covers the next tile
    assert any(p % 8 == 0 and p % gc.TS for p in st) and sum(1 <= p % 8 <= 6 for p in st) >= 2      # a lane-block border; inside lane blocks
    assert sum(lay.offsets[lay.group_at(p) + 1] // gc.TS > p // gc.TS for p in st) >= 4             # carries between the first row and the rows that read it


@pytest.mark.parametrize("dt", MUT_DTYPES, ids=ex.nm)
def test_ratiow_without_the_short_group_rule_is_refused(oracle, dt):
    """a group of at most w rows scanned as if it were longer (w = 2 cannot tell: both forms divide rows 0 and 1 by row 0)"""
    lay = gc.layout("borders")
    flat = column_of(lay, dt, "ratiow")
    for w in (7, 100):
        long_form = lambda v: oracle.scan(ck.SCAN_RATIOW, np.concatenate([v, np.ones(w + 1, v.dtype)]), w)[:len(v)]
        got = gc.compose_flat(lay, flat, long_form, gc.out_dtype(oracle, "ratiow", dt))
        assert refuses("ratiow", lay, flat, w, got, gc.expected(oracle, lay, "ratiow", flat, w)), w


@pytest.mark.parametrize("dt", MUT_DTYPES, ids=ex.nm)
@pytest.mark.parametrize("lname", gc.LAYOUTS)
def test_a_leak_from_a_poisoned_group_is_refused(oracle, lname, dt):
    """the composition of the poisoned column with one row of each neighbour handed to every group, against the twin's: the first rows of a
    group see the last row of the group in front, aggnext's last row the first row of the group behind"""
    lay = gc.layout(lname)
    bad, twin = gc.poisoned(lay, dt)
    for name in gc.OPS:
        if not usable(name, dt):
            continue
        w = window_of(name, dt, lay)
        honest, good = gc.expected(oracle, lay, name, bad, w), truth(oracle, lay, name, twin, w)
        want = gc.expected(oracle, lay, name, twin, w)
        gc.check_isolated(name, lay, w, honest, want)
        gc.check(name, lay, twin, w, good, want)
        leaks = [gc.expected(oracle, lay, name, x, w, left=1, right=1) for x in (bad, twin)]
        with pytest.raises(AssertionError):
            gc.check_poisoned(name, lay, twin, w, leaks[0], leaks[1], want)


@pytest.mark.parametrize("dt", [np.dtype(np.int64), np.dtype(np.uint64)], ids=ex.nm)
def test_a_running_sum_cut_to_64_bits_is_refused(oracle, dt):
    lay = gc.layout("borders")
    for cname, flat in gc.one_sign_columns(lay, dt):
        for name, w in (("sums", 0), ("sumw", 100), ("sumw", gc.first_hbm_w(gc.sum_route, dt))):
            want = gc.expected(oracle, lay, name, flat, w)
            got = want.copy()
            got["hi"] = (got["lo"].view(np.int64) >> 63) if dt.kind == "i" else 0
            assert refuses(name, lay, flat, w, got, want), (cname, name, w)
