"""Named cases of the as-of join (aqg_join_asof), each the smallest shape at which its mistake shows, shared by the model's tests
(tests/test_asof_model.py) and the device's (tests/test_gpu_asof.py).  A case is (build_cols, build_on, probe_cols, probe_on, routes):
key columns in the (tag, data) format of tests/join_keys_model.py, the `on` columns as numpy arrays of one dtype, and the route bits
aqg_join_asof_last must report -- LDS when the ordered build side (nb images of 4 or 8 bytes, nb row ids, G + 1 offsets) fits 48 KB
under at least 2^16 probe rows, else HBM; NOKEYS without key columns; PRESORTED when the build side's `on` is non-decreasing with
its NaNs last."""
import numpy as np

import checker as ck
from asof_model import HBM, LDS, NOKEYS, PRESORTED

_CASES = None


def _key(a, dtype=np.int32):
    a = np.asarray(a, dtype=dtype)
    return (ck.NP2TAG[a.dtype], a)


def _group_sizes():
    """groups of 1, 2, 2^k - 1, 2^k, 2^k + 1 rows (k up to 11); `on` in runs of two equal values, build side shuffled.  Per group the
    probe asks below the first, at the first, at the last, above the last, at every run and between every two runs (odd values)"""
    rng = np.random.default_rng(11)
    sizes = sorted({1, 2} | {(1 << k) + d for k in range(2, 12) for d in (-1, 0, 1)})
    bk, bo, pk, po = [], [], [], []
    for g, s in enumerate(sizes):
        on = 10 * (np.arange(s) // 2) + 100 * g                  # neighbouring groups overlap in `on`
        bk.append(np.full(s, 7 * g + 3)); bo.append(on)
        q = np.concatenate([[on[0] - 1, on[0], on[-1], on[-1] + 1], rng.choice(on, min(s, 12)), rng.choice(on, min(s, 12)) + 5])
        pk.append(np.full(len(q), 7 * g + 3)); po.append(q)
    bk, bo, pk, po = (np.concatenate(x) for x in (bk, bo, pk, po))
    sb, sp = rng.permutation(len(bk)), rng.permutation(len(pk))
    return [_key(bk[sb])], bo[sb].astype(np.int64), [_key(pk[sp])], po[sp].astype(np.int64), HBM


def _straddle():
    """group g's largest `on` above group g+1's smallest (groups 0 -> 1, 2 -> 3) and the reverse (1 -> 2): a segment bound off by one
    returns a row of the neighbour, and the probes below and above every segment make that row a wrong one"""
    lo = [100, 0, 200, 50]
    bk = np.repeat(np.arange(4), 10)
    bo = np.concatenate([l + 2 * np.arange(10) for l in lo])
    pk = np.repeat(np.arange(4), 8)
    po = np.concatenate([[-1000, l - 1, l, l + 1, l + 9, l + 18, l + 19, 1000] for l in lo])
    return [_key(bk)], bo.astype(np.int64), [_key(pk)], po.astype(np.int64), HBM


def _all_ties():
    rng = np.random.default_rng(12)
    return ([_key(rng.integers(0, 3, 3000))], np.full(3000, 7, np.int32), [_key(rng.integers(0, 4, 600))], rng.integers(6, 9, 600).astype(np.int32),
            HBM | PRESORTED)


def _absent_keys():
    """half of the probe keys are not on the build side; group 0 (key 5) has partners for every `on`, so a probe sent there finds one"""
    rng = np.random.default_rng(13)
    bk = np.concatenate([np.full(20, 5), rng.integers(6, 12, 80)])
    pk = np.concatenate([rng.integers(5, 12, 100), rng.integers(100, 200, 100)])
    return [_key(bk)], rng.integers(0, 50, 100).astype(np.int16), [_key(pk)], rng.integers(-5, 55, 200).astype(np.int16), HBM


def _nokeys(sort):
    rng = np.random.default_rng(14)
    bo = rng.integers(0, 400, 1000).astype(np.float64) / 4
    return [], np.sort(bo) if sort else bo, [], rng.integers(-8, 408, 777).astype(np.float64) / 4, HBM | NOKEYS | (PRESORTED if sort else 0)


def _tuple_case(kinds, seed):
    """a tuple of key columns from a small domain each, so that tuples repeat; a floating key column holds NaN and both zeros"""
    rng = np.random.default_rng(seed)
    nb, npr = 700, 900

    def col(kind, n):
        if kind == "f64":
            return (ck.DOUBLE, rng.choice(np.array([0.0, -0.0, 1.5, np.nan, -2.0]), n))
        dt = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "u64": np.uint64}[kind]
        return _key(rng.integers(0, 4, n).astype(dt) * dt(np.iinfo(dt).max // 3), dt)
    return [col(k, nb) for k in kinds], rng.integers(0, 60, nb).astype(np.uint16), [col(k, npr) for k in kinds], rng.integers(0, 60, npr).astype(np.uint16), HBM


def _np_case(npr, nb=1000, on_dtype=np.int64):
    """ten symbols over a shuffled build side of nb rows; 2^16 + 3 probe rows take the LDS route (1000 rows: 12 KB of images and ids)"""
    rng = np.random.default_rng(15 + npr % 97)
    big = npr >= 1 << 16
    return ([_key(rng.integers(0, 10, nb), np.uint32)], rng.integers(0, 300, nb).astype(on_dtype),
            [_key(rng.integers(0, 11, npr), np.uint32)], rng.integers(-3, 303, npr).astype(on_dtype), LDS if big else HBM)


def _ends(dtype):
    """`on` at the ends of its type, on both sides"""
    rng = np.random.default_rng(16)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        fi = np.finfo(dt)
        vals = np.array([-np.inf, -fi.max, -1.0, -fi.tiny, -fi.smallest_subnormal, -0.0, 0.0, fi.smallest_subnormal, fi.tiny, 1.0, fi.max, np.inf, np.nan], dt)
    else:
        ii = np.iinfo(dt)
        mid = (int(ii.max) + int(ii.min)) // 2
        vals = np.array([ii.min, ii.min + 1, mid - 1, mid, mid + 1, mid + 2, ii.max - 1, ii.max], dt)   # unsigned: around 2^(bits-1), where a signed compare turns over
    bo, po = rng.choice(vals, 300), np.concatenate([vals, rng.choice(vals, 100)])
    return [_key(rng.integers(0, 3, len(bo)))], bo, [_key(rng.integers(0, 3, len(po)))], po, HBM


def _sorted_case(kind):
    rng = np.random.default_rng(17)
    nb = 2000
    bo = np.sort(rng.integers(0, 500, nb)).astype(np.float64)
    routes = HBM | PRESORTED
    if kind == "swapped":
        i = int(np.nonzero(bo[:-1] < bo[1:])[0][nb // 300])
        bo[i], bo[i + 1] = bo[i + 1], bo[i]
        routes = HBM
    elif kind == "nan_middle":
        bo[nb // 2] = np.nan
        routes = HBM
    elif kind == "nan_last":
        bo[-3:] = np.nan
    return [_key(rng.integers(0, 20, nb))], bo, [_key(rng.integers(0, 21, 1500))], rng.integers(-2, 502, 1500).astype(np.float64), routes


def _hbm_big():
    """2^17 build rows: 1.5 MB of images and ids, past the LDS route at any probe size; a time-ordered side"""
    rng = np.random.default_rng(18)
    nb, npr = 1 << 17, 5000
    return ([_key(rng.integers(0, 4096, nb), np.uint32)], np.sort(rng.integers(0, 1 << 40, nb)).astype(np.int64),
            [_key(rng.integers(0, 4100, npr), np.uint32)], rng.integers(0, 1 << 40, npr).astype(np.int64), HBM | PRESORTED)


def cases():
    global _CASES
    if _CASES is None:
        c = {"group_sizes": _group_sizes(), "straddle": _straddle(), "all_ties": _all_ties(), "absent_keys": _absent_keys(),
             "nokeys": _nokeys(False), "nokeys_presorted": _nokeys(True),
             "tuple2_packed": _tuple_case(("i32", "i32"), 21), "tuple3_packed": _tuple_case(("i8", "i16", "i32"), 22),
             "tuple2_wide": _tuple_case(("i64", "i32"), 23), "tuple3_wide_f64": _tuple_case(("f64", "u64", "i8"), 24),
             "lds_i64": _np_case((1 << 16) + 3), "lds_i32": _np_case((1 << 16) + 3, on_dtype=np.int32), "hbm_big": _hbm_big()}
        for n in (1, 2, 3, 5):
            c["np_%d" % n] = _np_case(n, nb=64)
        for dt in ("int64", "uint64", "int8", "uint8", "float64", "float32"):
            c["ends_" + dt] = _ends(dt)
        for kind in ("sorted", "swapped", "nan_middle", "nan_last"):
            c["build_" + kind] = _sorted_case(kind)
        _CASES = c
    return _CASES


ON_DTYPES = (np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64)
KEY_SPECS = ((), ("i32",), ("i8", "i16"), ("i64", "i32"), ("u64",), ("f64", "i32"))


def random_sides(seed, max_n):
    """seeded random sides: (build_cols, build_on, probe_cols, probe_on, direction, strict); a small `on` domain (many ties), floating
    columns with NaN and both zeros, one side in time order every third seed"""
    rng = np.random.default_rng(1000 + seed)
    nb, npr = int(rng.integers(0, max_n + 1)), int(rng.integers(1, max_n + 1))
    spec = KEY_SPECS[seed % len(KEY_SPECS)]
    dt = np.dtype(ON_DTYPES[(seed // 2) % len(ON_DTYPES)])
    dom = int(rng.integers(2, 40))

    def on(n):
        v = rng.integers(0, dom, n)
        if dt.kind == "f":
            a = (v - dom // 2).astype(dt) / 2
            a[rng.random(n) < 0.05] = np.nan
            a[rng.random(n) < 0.05] = -0.0
            return a
        if dt.kind == "i":
            return (v - dom // 2).astype(dt)
        return (np.iinfo(dt).max // 2 - dom // 2 + v).astype(dt)

    def keys(n):
        out = []
        for k in spec:
            if k == "f64":
                out.append((ck.DOUBLE, rng.choice(np.array([0.0, -0.0, 2.5, np.nan]), n)))
            else:
                d = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "u64": np.uint64}[k]
                out.append(_key(rng.integers(0, 3, n).astype(d) * d(np.iinfo(d).max // 2), d))
        return out
    bo = on(nb)
    if seed % 3 == 0:
        bo = np.sort(bo)                                         # NaNs last
    return keys(nb), bo, keys(npr), on(npr), int(rng.integers(0, 2)), bool(rng.integers(0, 2))
