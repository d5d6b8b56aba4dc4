"""aqg_scan_ema / aqg_grouped_ema / aqg_grouped_ema_flat / aqg_decay_from_times (ema.hip): exponential moving averages of a column and
of every group of a build.  Everything goes through the C-ABI and is held to the exact model of tests/ema_model.py under the DERIVED
bounds of DESIGN.md section 4.15 -- |got - exact| <= 4 (i + 2) u M_i (recursive) / 9 (i + 2) u M_i (adjusted), u = 2^-53 -- for every
finite row; rows from a slice's first non-finite row on are checked for ~isfinite only.  Slices too long for the exact model are held
to its extended-precision evaluation, whose own error is taken OFF the bound.  The cases live in tests/ema_cases.py on the tile
geometry read from the code; tests/test_ema_model.py shows on the CPU that they refuse every planted mistake."""
import functools

import mpmath
import numpy as np
import pytest

import ema_cases as ec
import ema_model as em
from aquery2_amd.capi import DATE, EMA_ADJUSTED, EMA_RECURSIVE, INT128, TIME, UINT64, UINT128

pytestmark = pytest.mark.gpu
ERR_DTYPE, ERR_ARG = 2, 3
assert (EMA_RECURSIVE, EMA_ADJUSTED) == (em.RECURSIVE, em.ADJUSTED)


@pytest.fixture(scope="module")
def dev():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


def hold(got, ref, mode, what):
    """the device's answer against a reference (ema_model.Reference): the bound on the finite rows, ~isfinite behind a poisoned one"""
    assert got.shape == ref.M.shape and got.dtype == np.float64, what
    bad = ref.poisoned
    assert not np.isfinite(got[bad]).any(), (what, "a row behind its slice's first non-finite row came out finite")
    ok = ~bad
    err = np.abs(got[ok].astype(np.longdouble) - ref.y[ok]).astype(np.float64)
    allow = em.bound(mode, ref.M, ref.pos)[ok] - ref.err[ok]
    worst = float(np.max(err / np.maximum(allow, 1e-300))) if ok.any() else 0.0
    print("%s: worst |got - exact| / bound = %.3g" % (what, worst))
    assert np.isfinite(got[ok]).all() and np.all(err <= allow), (what, worst, int(np.argmax(err / np.maximum(allow, 1e-300))))


def run_case(dev, c, gb=None):
    if c.kind == "flat":
        return {"flat": dev.ema(c.x, alpha=c.alpha, decay=c.decay, mode=c.mode)}
    return {"row": dev.grouped_ema(gb, c.x_row, alpha=c.alpha, decay=c.decay_row, mode=c.mode),
            "flat": dev.grouped_ema(gb, c.x, alpha=c.alpha, decay=c.decay, mode=c.mode, flat=True)}


FLAT = ec.flat_cases()
GROUPED = ec.grouped_cases()


@pytest.mark.parametrize("dt", sorted({c.dtype.name for c in FLAT}))
def test_flat_grid(dev, dt):
    """every n of the grid (lane-block, wave and tile edges), both modes, constant alpha and the decay columns (zeros: a hard restart
    inside the column; ones; denormal products)"""
    cases = [c for c in FLAT if c.dtype.name == dt]
    assert cases
    for c in cases:
        hold(run_case(dev, c)["flat"], ec.reference(c), c.mode, c.name)


@pytest.mark.parametrize("layout", sorted({c.name.split("-")[1] for c in GROUPED}))
def test_grouped(dev, layout):
    """group starts on and beside tile and lane-block borders, a group over three tiles beside groups of one row, one group, every
    row its own, G on both sides of 256, and a poisoned group between two tame ones -- through both grouped entries"""
    cases = [c for c in GROUPED if c.name.split("-")[1] == layout]
    for c in cases:
        gb = dev.groupby_build([c.keys_row])
        assert gb.ngroups == len(c.starts)
        assert np.array_equal(dev.group_offsets(gb)[:len(c.starts)], c.starts)
        ref = ec.reference(c)
        if layout.startswith("poison"):
            assert ref.poisoned.any() and not ref.poisoned[:c.starts[1]].any() and not ref.poisoned[c.starts[2]:].any()
        for entry, got in run_case(dev, c, gb).items():
            hold(got, ref, c.mode, c.name + "/" + entry)
        gb.destroy()


# ---- the aggregate scan's second round: millions of rows ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_column(n):
    """values every dtype of the grid holds (0 .. 126), so that one reference serves them all"""
    return np.random.default_rng(n).integers(0, 127, size=n, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def big_decay(n):
    d = np.random.default_rng(n + 1).uniform(0.9, 1.0, size=n)         # long memories: the weights stay alive across many tiles
    d[::100003] = 0.0
    return d


def big_reference(n, mode, decayed):
    return em.reference_ema(big_column(n), None, mode, alpha=None if decayed else 2.0 ** -20, decay=big_decay(n) if decayed else None)


@pytest.mark.parametrize("decayed", [False, True], ids=["alpha", "decay"])
@pytest.mark.parametrize("mode", [EMA_RECURSIVE, EMA_ADJUSTED], ids=["recursive", "adjusted"])
@pytest.mark.parametrize("n", ec.BIG_N)
def test_flat_big(dev, n, mode, decayed):
    """CH TS - 1, CH TS, CH TS + 1 and 2 CH TS + 3 rows: the second round of the aggregate scan; alpha = 2^-20 keeps every weight alive"""
    ref = big_reference(n, mode, decayed)
    dd = dev.to_device(big_decay(n)) if decayed else None
    for k, dt in enumerate(ec.GRID_DTYPES):
        got = dev.ema(big_column(n).astype(dt), alpha=2.0 ** -20, decay=dd, mode=mode)
        hold(got, ref, mode, "big-%s-n%d-m%d-%s" % (np.dtype(dt).name, n, mode, "decay" if decayed else "alpha"))


# ---- reproducibility ---------------------------------------------------------------------------------------------------------------
def test_bit_reproducible(dev):
    """the same call twice into different buffers: byte-equal, flat and grouped, at 2 CH TS + 3 rows"""
    n = ec.BIG_N[-1]
    x = dev.to_device(np.random.default_rng(3).normal(size=n))
    dec = dev.to_device(big_decay(n))
    keys = np.repeat(np.arange(1000, dtype=np.int32), -(-n // 1000))[:n]
    gb = dev.groupby_build([keys])
    for mode in (EMA_RECURSIVE, EMA_ADJUSTED):
        for kw in ({"alpha": 2.0 ** -20}, {"decay": dec}):
            a = dev.ema(x, mode=mode, **kw)
            b = dev.ema(x, mode=mode, **kw)
            assert a.tobytes() == b.tobytes()
            a = dev.grouped_ema(gb, x, mode=mode, flat=True, **kw)
            b = dev.grouped_ema(gb, x, mode=mode, flat=True, **kw)
            assert a.tobytes() == b.tobytes()
    a = dev.grouped_ema(gb, x, alpha=0.01)
    b = dev.grouped_ema(gb, x, alpha=0.01)
    assert a.tobytes() == b.tobytes()
    gb.destroy()


# ---- errors -----------------------------------------------------------------------------------------------------------------------
CANARY = 0x5EEDFACECAFEBEEF


def canary(dev, n):
    return dev.to_device(np.full(n, CANARY, np.uint64))


def untouched(buf):
    return bool((buf.to_host() == np.uint64(CANARY)).all())


def test_errors_write_nothing(dev):
    n = 1000
    x = dev.to_device(np.arange(n, dtype=np.int32))
    dec = dev.to_device(np.full(n, 0.5))
    keys = dev.to_device((np.arange(n) % 7).astype(np.int32))
    gb = dev.groupby_build([keys])
    agg = dev.groupby_agg([keys], [0], [x])
    out = canary(dev, n)
    lib, ctx = dev.lib, dev.ctx

    def flat(mode, t, xp, nn, alpha, dp, op):
        return lib.aqg_scan_ema(ctx, mode, t, xp, nn, alpha, dp, op)

    for alpha in (0.0, -0.1, 1.5, float("nan")):
        assert flat(0, x.tag, x.ptr, n, alpha, None, out.ptr) == ERR_ARG
        assert lib.aqg_grouped_ema(ctx, gb.h, 0, x.tag, x.ptr, alpha, None, out.ptr) == ERR_ARG
        assert lib.aqg_grouped_ema_flat(ctx, gb.h, 1, x.tag, x.ptr, alpha, None, out.ptr) == ERR_ARG
    assert flat(0, x.tag, x.ptr, n, float("nan"), dec.ptr, out.ptr) == 0          # alpha is ignored beside a decay column
    out = canary(dev, n)
    for mode in (-1, 2):
        assert flat(mode, x.tag, x.ptr, n, 0.5, None, out.ptr) == ERR_ARG
        assert lib.aqg_grouped_ema_flat(ctx, gb.h, mode, x.tag, x.ptr, 0.5, None, out.ptr) == ERR_ARG
    for t in (INT128, UINT128, DATE):
        assert flat(0, t, x.ptr, n, 0.5, None, out.ptr) == ERR_DTYPE
        assert lib.aqg_grouped_ema(ctx, gb.h, 0, t, x.ptr, 0.5, None, out.ptr) == ERR_DTYPE
    assert lib.aqg_decay_from_times(ctx, INT128, x.ptr, n, 1.0, out.ptr) == ERR_DTYPE
    assert lib.aqg_grouped_ema(ctx, agg.h, 0, x.tag, x.ptr, 0.5, None, out.ptr) == ERR_ARG          # not a handle of aqg_groupby_build
    assert lib.aqg_grouped_ema_flat(ctx, agg.h, 0, x.tag, x.ptr, 0.5, None, out.ptr) == ERR_ARG
    assert flat(0, x.tag, None, n, 0.5, None, out.ptr) == ERR_ARG
    assert flat(0, x.tag, x.ptr, n, 0.5, None, None) == ERR_ARG
    for h in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.aqg_decay_from_times(ctx, x.tag, x.ptr, n, h, out.ptr) == ERR_ARG
    assert untouched(out)
    # out overlapping an input: the column itself, its tail, the decay column
    xd = canary(dev, n)
    assert flat(0, UINT64, xd.ptr, n, 0.5, None, xd.ptr) == ERR_ARG
    assert flat(0, UINT64, xd.ptr, n, 0.5, None, xd.ptr + 8 * (n - 1)) == ERR_ARG
    assert flat(0, x.tag, x.ptr, n, 0.5, xd.ptr, xd.ptr) == ERR_ARG
    assert lib.aqg_grouped_ema_flat(ctx, gb.h, 0, UINT64, xd.ptr, 0.5, None, xd.ptr) == ERR_ARG
    assert lib.aqg_decay_from_times(ctx, UINT64, xd.ptr, n, 1.0, xd.ptr) == ERR_ARG
    assert untouched(xd)
    # nothing to do
    assert flat(0, x.tag, None, 0, 0.5, None, None) == 0
    assert lib.aqg_decay_from_times(ctx, x.tag, None, 0, 1.0, None) == 0
    empty = dev.groupby_build([np.zeros(0, np.int32)])
    assert lib.aqg_grouped_ema(ctx, empty.h, 0, x.tag, None, 0.5, None, None) == 0
    assert lib.aqg_grouped_ema_flat(ctx, empty.h, 0, x.tag, None, 0.5, None, None) == 0
    assert untouched(out)
    for h in (gb, agg, empty):
        h.destroy()


# ---- aqg_decay_from_times -----------------------------------------------------------------------------------------------------------
def ulp(v):
    return np.spacing(np.abs(v))


def decay_exact(stamps, halflife):
    """2^(-|dt| / halflife) at 60 digits (stamps: python ints or floats, exact), rounded to double by the caller's comparison"""
    mpmath.mp.dps = 60
    out = [mpmath.mpf(1)]
    for a, b in zip(stamps[1:], stamps[:-1]):
        out.append(mpmath.power(2, -abs(mpmath.mpf(a) - mpmath.mpf(b)) / mpmath.mpf(halflife)))
    return out


def hold_decay(got, want, what):
    """2 ulp of the result: 1 ulp is the documented accuracy of the device library's double exp2, one more rounding from the quotient"""
    assert got[0] == 1.0
    worst = 0.0
    for g, w in zip(got, want):
        e = abs(mpmath.mpf(float(g)) - w)
        u = mpmath.mpf(float(ulp(float(w)))) if w > mpmath.mpf(2) ** -1000 else mpmath.mpf(2) ** -1074
        worst = max(worst, float(e / u))
    print("%s: worst error %.3f ulp" % (what, worst))
    assert worst <= 2.0, (what, worst)


def test_decay_from_times(dev):
    rng = np.random.default_rng(11)
    n = 3000                                                   # more than one workgroup's stride
    # int64 nanosecond stamps near 2^62: the difference is taken in integers (the doubles next to 2^62 are 1024 apart)
    t = (2 ** 62 + np.cumsum(rng.integers(1, 3_000_000_000, size=n))).astype(np.int64)
    for order, name in ((t, "ascending"), (t[::-1].copy(), "descending")):
        h = 1.5e9
        hold_decay(dev.decay_from_times(order, h), decay_exact([int(v) for v in order], h), "int64 ns " + name)
    u = (2 ** 63 + np.cumsum(rng.integers(1, 1000, size=n)).astype(np.uint64)).astype(np.uint64)
    hold_decay(dev.decay_from_times(u, 37.0), decay_exact([int(v) for v in u], 37.0), "uint64")
    d = np.cumsum(rng.uniform(0.0, 2.0, size=n))
    hold_decay(dev.decay_from_times(d, 0.7), decay_exact([float(v) for v in d], 0.7), "double")
    f = np.cumsum(rng.uniform(0.0, 2.0, size=n)).astype(np.float32)[::-1].copy()
    hold_decay(dev.decay_from_times(f, 3.0), decay_exact([float(v) for v in f], 3.0), "float descending")
    i8 = rng.integers(-128, 127, size=n).astype(np.int8)
    hold_decay(dev.decay_from_times(i8, 16.0), decay_exact([int(v) for v in i8], 16.0), "int8 unordered")
    # AQG_DATE {day, month, year}: differences in days; AQG_TIME {ms, seconds, minutes, hours, pad}: in milliseconds
    import datetime
    days = np.cumsum(rng.integers(0, 400, size=n)) + datetime.date(1899, 12, 25).toordinal()
    dates = np.array([(x.day, x.month, x.year & 0xFF, (x.year >> 8) & 0xFF) for x in map(datetime.date.fromordinal, days.tolist())], np.uint8)
    hold_decay(dev.decay_from_times(dev.key_col(DATE, dates), 30.0), decay_exact([int(v) for v in days], 30.0), "DATE")
    ms = np.sort(rng.integers(0, 86_400_000, size=n))
    times = np.zeros((n, 8), np.uint8)
    times[:, :4] = (ms % 1000).astype("<u4").view(np.uint8).reshape(n, 4)
    times[:, 4], times[:, 5], times[:, 6] = (ms // 1000) % 60, (ms // 60_000) % 60, ms // 3_600_000
    hold_decay(dev.decay_from_times(dev.key_col(TIME, times), 5000.0), decay_exact([int(v) for v in ms], 5000.0), "TIME")


def test_time_decayed_average_by_group(dev):
    """the use the entry is for: decay_from_times over the flat layout feeds aqg_grouped_ema_flat -- group borders need no care, since a
    group's first decay is not read; the grouped form of the entry writes 1 there"""
    c = next(c for c in GROUPED if c.name.startswith("grouped-edges-") and c.decay is None and c.mode == em.ADJUSTED)
    rng = np.random.default_rng(12)
    t_row = np.cumsum(rng.integers(1, 50, size=len(c.x))).astype(np.int64)
    gb = dev.groupby_build([c.keys_row])
    t_flat = dev.grouped_flatten(gb, t_row)
    dec = dev.decay_from_times(t_flat, 20.0)
    got = dev.grouped_ema(gb, c.x, decay=dec, mode=em.ADJUSTED, flat=True)
    hold(got, em.reference_ema(c.x, c.starts, em.ADJUSTED, decay=dec), em.ADJUSTED, "time-decayed by group")
    decg = dev.decay_from_times(t_flat, 20.0, gb=gb)
    first = np.zeros(len(dec), bool)
    first[c.starts] = True
    assert np.all(decg[first] == 1.0) and np.array_equal(decg[~first], dec[~first])
    gb.destroy()


def test_emitted_group_loop(tmp_path):
    """tests/emitted/ema.cpp over host_main's synthetic dataset (2e5 rows): `ema(0.25, c[vecs[g]], col[g])` and
    `ewmad(decayt(40, t[vecs[g]]), c[vecs[g]], col[g])` in the generated group loop cost ONE aqg_grouped_ema_flat each, at 1000 groups
    and at 10; a `subvec(0, 2)` view of the temporary takes the per-group path and gives the per-group answer"""
    import subprocess
    from test_gpu_emitted import EM, run
    from test_gpu_quantiles import _synthetic
    import quantile_model as qm
    subprocess.check_call(["make", "-C", EM, "build/ema.so", "build/host_main"], stdout=subprocess.DEVNULL)
    a, c = _synthetic()
    run("ema.so", "synthetic", "dll_ema_flat", "dll_ema_group", "dll_ema_group10", cwd=str(tmp_path))
    n = len(c)
    whole = np.zeros(n, np.int64)
    for k, mode in enumerate((em.RECURSIVE, em.ADJUSTED)):
        ref = em.reference_ema(c, None, mode, alpha=0.25)
        hold(np.fromfile(tmp_path / ("emaf.out.%d" % k), np.float64), ref, mode, "emitted flat m%d" % mode)
    t = np.fromfile(tmp_path / "ema.t", np.int32)
    assert len(t) == n and np.all(np.diff(t) >= 1)
    for name, key, G in (("emag", a, 1000), ("emag10", a % 10, 10)):
        gid, ng = qm.first_occurrence_ids(key)
        assert ng == G
        # the group loop's row lists: groups in first-occurrence order, a group's rows in descending row id (the flat layout)
        order = np.lexsort((-np.arange(n), gid))
        starts = np.flatnonzero(np.diff(gid[order], prepend=-1))
        first = np.full(G, n, np.int64)
        np.minimum.at(first, gid, np.arange(n))
        assert np.array_equal(np.fromfile(tmp_path / (name + ".out.0"), np.int32), key[first])
        cf, tf = c[order], t[order]
        hold(np.fromfile(tmp_path / (name + ".out.1"), np.float64), em.reference_ema(cf, starts, em.RECURSIVE, alpha=0.25), em.RECURSIVE, name + " ema")
        # the header layer's decay column (one call for all groups, memoised: the very column ewmad read), held to the exact power
        # like test_decay_from_times, then given to the model as the decays it is
        dec = np.fromfile(tmp_path / (name + ".out.4"), np.float64)
        head = np.zeros(n, bool)
        head[starts] = True
        assert len(dec) == n and np.all(dec[head] == 1.0)
        steps = np.abs(np.diff(tf.astype(np.int64), prepend=0))
        table = [mpmath.power(2, -mpmath.mpf(v) / 40) for v in range(int(steps[~head].max()) + 1)]
        tab_f = np.array([float(v) for v in table])
        assert np.all(np.abs(dec[~head] - tab_f[steps[~head]]) <= 2 * np.spacing(tab_f[steps[~head]]))
        hold(np.fromfile(tmp_path / (name + ".out.2"), np.float64), em.reference_ema(cf, starts, em.ADJUSTED, decay=dec), em.ADJUSTED, name + " ewmad")
        # the two-row views, one per group, each the per-group answer of its first two rows
        sub = np.fromfile(tmp_path / (name + ".out.3"), np.float64)
        counts = np.diff(np.append(starts, n))
        assert len(sub) == int(np.minimum(counts, 2).sum())
        want, k = [], 0
        for s0, cnt in zip(starts, counts):
            want.append(float(cf[s0]))
            if cnt >= 2:
                want.append(0.25 * float(cf[s0 + 1]) + 0.75 * float(cf[s0]))
        assert np.array_equal(sub, np.array(want))
        calls, groups = (int(v) for v in (tmp_path / (name + ".calls")).read_text().split())
        assert groups == G and calls == 2, "one grouped call per grouped form, whatever the number of groups"
