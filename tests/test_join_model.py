"""The join model (tests/join_model.py) against the oracle's C restatement of the pair join and against plain dict loops.  No GPU."""
import numpy as np
import pytest

import join_model as jm

KEY_DTYPES = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64]


def edge_keys(dt):
    """the keys a 64-bit key image could confuse: -1 / the all-ones word, the type's ends and their neighbours, zero"""
    info = np.iinfo(dt)
    vals = {int(info.min), int(info.min) + 1, int(info.max), int(info.max) - 1, 0, 1}
    if info.min < 0:
        vals |= {-1, -2}
    return sorted(vals)


def columns(rng, dt, nb, npr):
    """build and probe columns drawn from the edge keys and a few random ones: duplicates on both sides, misses on the probe side"""
    info = np.iinfo(dt)
    pool = np.array(edge_keys(dt) + rng.integers(info.min, info.max, 12, dtype=dt, endpoint=True).tolist(), dtype=dt)
    build = rng.choice(pool[:-4], nb).astype(dt)                  # the last four keys of the pool: probe-side only
    probe = rng.choice(pool, npr).astype(dt)
    edges = np.array(edge_keys(dt), dtype=dt)
    if nb >= 40:                                                  # every edge key on the build side, at scattered rows, some twice
        build[rng.permutation(nb)[:len(edges)]] = edges
    if npr >= 25:
        probe[rng.permutation(npr)[:len(edges)]] = edges
    return build, probe


@pytest.mark.parametrize("dt", KEY_DTYPES, ids=lambda d: np.dtype(d).name)
def test_pairs_match_the_oracle(oracle, dt):
    rng = np.random.default_rng(21)
    for nb, npr in ((0, 0), (0, 9), (9, 0), (1, 1), (40, 25), (300, 1000), (2000, 33)):
        build, probe = columns(rng, dt, nb, npr)
        if nb >= 40:
            assert {int(np.iinfo(dt).min), int(np.iinfo(dt).max)} <= set(build.tolist())
            assert np.iinfo(dt).min == 0 or -1 in build.tolist()
        pr, br = jm.pairs(build, probe)
        opr, obr = oracle.join_pairs(build, probe)
        assert pr.dtype == br.dtype == np.uint32
        assert np.array_equal(pr, opr) and np.array_equal(br, obr), (nb, npr)
        assert jm.count(build, probe) == len(opr) and isinstance(jm.count(build, probe), int)
    # every edge key against every edge key, once each: equality is by value, -1 is not the unsigned maximum of a narrower type
    keys = np.array(edge_keys(dt), dtype=dt)
    pr, br = jm.pairs(keys, keys[::-1].copy())
    assert np.array_equal(pr, np.arange(len(keys))) and np.array_equal(br, np.arange(len(keys))[::-1])


@pytest.mark.parametrize("dt", KEY_DTYPES, ids=lambda d: np.dtype(d).name)
def test_lookup_matches_a_dict_loop(dt):
    rng = np.random.default_rng(22)
    for nb, npr in ((0, 5), (5, 0), (1, 3), (60, 200), (700, 50)):
        build, probe = columns(rng, dt, nb, npr)
        first = {}
        for r, k in enumerate(build.tolist()):
            first.setdefault(k, r)
        want = np.array([first.get(k, jm.NONE) for k in probe.tolist()], dtype=np.uint32)
        got = jm.lookup(build, probe)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (nb, npr)


def test_bool_keys_are_their_values():
    build = np.array([True, False, True, True])
    probe = np.array([False, True, False])
    assert jm.lookup(build, probe).tolist() == [1, 0, 1]
    pr, br = jm.pairs(build, probe)
    assert pr.tolist() == [0, 1, 1, 1, 2] and br.tolist() == [1, 0, 2, 3, 1]
    assert jm.count(build, probe) == 5


@pytest.mark.parametrize("vdt,wdt", [(np.int32, np.int32), (np.uint32, np.uint32), (np.uint32, np.int32), (np.int32, np.uint32)])
def test_star_sum_matches_a_dict_loop(vdt, wdt):
    rng = np.random.default_rng(23)
    ext = lambda d: [0, 1, int(np.iinfo(d).max), int(np.iinfo(d).min), int(np.iinfo(d).max) - 1]
    for n, nb in ((0, 4), (5, 0), (1, 1), (400, 12), (3000, 40)):
        dim_key = rng.choice(np.array([-1, 0, 5, 7, 2**31 - 1, -2**31, 9], dtype=np.int32), nb)       # duplicates: the lowest row wins
        dim_w = rng.choice(np.array(ext(wdt) + [3, 1000], dtype=wdt), nb)
        fk = rng.choice(np.array([-1, 0, 5, 7, 2**31 - 1, -2**31, 9, 11, -3], dtype=np.int32), n)  # 11 and -3 never have a partner
        gkey = rng.choice(np.array([0, 2**32 - 1, 2**31, 17, 2**31 - 1], dtype=np.uint32), n)
        val = rng.choice(np.array(ext(vdt) + [2, 77], dtype=vdt), n)
        first = {}
        for r, k in enumerate(dim_key.tolist()):
            first.setdefault(k, r)
        want, first_row = {}, {}
        for r, (f, g, v) in enumerate(zip(fk.tolist(), gkey.tolist(), val.tolist())):
            if f in first:
                want[g] = want.get(g, 0) + v * int(dim_w[first[f]])
                first_row.setdefault(g, r)
        keys, rows, sums = jm.star_sum(dim_key, dim_w, fk, gkey, val)
        assert keys.dtype == gkey.dtype and rows.dtype == np.uint32
        assert keys.tolist() == list(want)                              # dicts keep first-occurrence order
        assert rows.tolist() == [first_row[k] for k in want]
        assert sums == [want[k] for k in want] and all(isinstance(s, int) for s in sums)


def test_star_sum_is_exact_at_the_products_limits():
    n = (1 << 20) + 5
    one = lambda dt, v, m=n: np.full(m, v, dtype=dt)
    for vdt, v, wdt, w in ((np.int32, -2**31, np.int32, -2**31), (np.uint32, 2**32 - 1, np.uint32, 2**32 - 1), (np.int32, -2**31, np.uint32, 2**32 - 1),
                           (np.uint32, 2**32 - 1, np.int32, -2**31)):
        keys, rows, sums = jm.star_sum(one(np.int32, 5, 3), one(wdt, w, 3), one(np.int32, 5), one(np.int32, 1), one(vdt, v))
        assert keys.tolist() == [1] and rows.tolist() == [0] and sums == [n * v * w]


def test_model_at_the_suites_largest_shape():
    """1.1e6 rows through all three, the pair count consistent with the pairs (no time is asserted: the functions are sorts and
    searches over whole columns, a few tenths of a second each at this size)"""
    rng = np.random.default_rng(24)
    build = rng.integers(-2**63, 2**63 - 1, 1_100_000, dtype=np.int64)
    probe = np.concatenate([build[:50_000], rng.integers(-2**63, 2**63 - 1, 50_003, dtype=np.int64)])
    jm.lookup(build, probe)
    pr, br = jm.pairs(build, probe)
    assert jm.count(build, probe) == len(pr) >= 50_000
    fk = rng.integers(0, 5000, 1_100_000).astype(np.int32)
    keys, rows, sums = jm.star_sum(np.arange(4096, dtype=np.int32), np.arange(4096, dtype=np.int32), fk, (fk * 7 % 3000).astype(np.int32), fk)
    m = fk < 4096
    assert len(keys) == len(np.unique((fk * 7 % 3000)[m])) and sum(sums) == sum((fk[m].astype(np.int64) ** 2).tolist())
