"""aqg_sort_rows (sort.hip): stable multi-column device sort of row ids.  The expected order is numpy's stable np.lexsort over
the same order-preserving key images (ASC / DESC / NEG exactly as include/aqg.h states them), so the order of ties is checked too."""
import numpy as np
import pytest

import aquery2_amd
from aquery2_amd.capi import (BOOL, DOUBLE, FLOAT, I128, INT8, INT16, INT32, INT64, INT128, ORDER_ASC, ORDER_DESC, ORDER_NEG, STR,
                              U128, UINT8, UINT16, UINT32, UINT64, UINT128, AqgError, DevBuf)

pytestmark = pytest.mark.gpu

SMALL = 4096          # sort.hip SMALL: up to this many rows one workgroup sorts in LDS
CHUNK = 131072        # sort.hip CHUNK: rows per workgroup of a multi-launch pass
SIZES = [0, 1, 63, 64, 65, SMALL - 1, SMALL, SMALL + 1, CHUNK - 1, CHUNK, CHUNK + 1, 1_000_003]
NP = {INT8: np.int8, INT16: np.int16, INT32: np.int32, INT64: np.int64, UINT8: np.uint8, UINT16: np.uint16, UINT32: np.uint32,
      UINT64: np.uint64, FLOAT: np.float32, DOUBLE: np.float64, BOOL: np.bool_, INT128: I128, UINT128: U128}


@pytest.fixture(scope="module")
def dev():
    d = aquery2_amd.Device(0)
    yield d
    d.close()


def images(x, order):
    """order-preserving unsigned images of one key column, most significant first (a 16-byte key is two)"""
    x = np.asarray(x)
    if x.dtype.names:                                   # 128-bit: (lo, hi)
        lo, hi = x["lo"].astype(np.uint64), x["hi"].view(np.uint64).copy()
        if order == ORDER_NEG:
            lo = ~lo + np.uint64(1)
            hi = ~hi + (lo == 0).astype(np.uint64)
        if x.dtype == I128:
            hi ^= np.uint64(1 << 63)
        if order == ORDER_DESC:
            lo, hi = ~lo, ~hi
        return [hi, lo]
    if x.dtype == np.bool_:
        x = x.astype(np.uint8)
    if x.dtype.kind == "f":
        u = np.uint32 if x.itemsize == 4 else np.uint64
        b = x.view(u).copy()
        sign = u(1) << u(8 * x.itemsize - 1)
        b[x == 0] = 0
        b[np.isnan(x)] = x.dtype.type(np.nan).view(u) & ~sign
        b = np.where(b & sign, ~b, b | sign).astype(u)
        return [~b if order == ORDER_DESC else b]
    u = np.dtype(f"u{x.itemsize}")
    b = x.view(u).copy()
    if order == ORDER_NEG:
        b = (u.type(0) - b).astype(u)
    if x.dtype.kind == "i":
        b ^= u.type(1 << (8 * x.itemsize - 1))
    return [~b if order == ORDER_DESC else b]


def tagged(dev, keys):
    """keys as the call should see them: Device.to_device uploads a bool array as uint8, so a bool key is uploaded here and tagged BOOL"""
    out = []
    for k in keys:
        if isinstance(k, np.ndarray) and k.dtype == np.bool_:
            b = dev.to_device(k)
            b._tag = BOOL
            assert b.tag == BOOL
            k = b
        out.append(k)
    return out


def want_order(keys, orders, rows=None):
    rows = np.arange(len(keys[0]), dtype=np.uint32) if rows is None else np.asarray(rows, dtype=np.uint32)
    imgs = []
    for k, o in zip(keys, orders):
        imgs += [im[rows] for im in images(k, o)]
    if len(rows) == 0:
        return rows
    return rows[np.lexsort(imgs[::-1])]


def rand_col(rng, tag, n, distinct=None):
    if tag in (INT128, UINT128):
        a = np.zeros(n, dtype=NP[tag])
        a["lo"] = rng.integers(0, 2**64, n, dtype=np.uint64) if distinct is None else rng.integers(0, distinct, n).astype(np.uint64)
        hi = rng.integers(-2**63, 2**63, n, dtype=np.int64) if distinct is None else rng.integers(-2, 2, n).astype(np.int64)
        a["hi"] = hi if tag == INT128 else hi.view(np.uint64)
        return a
    if tag == BOOL:
        return rng.integers(0, 2, n).astype(np.bool_)
    if tag in (FLOAT, DOUBLE):
        v = rng.integers(-distinct, distinct, n) * 0.25 if distinct else rng.standard_normal(n) * 1e3
        return v.astype(NP[tag])
    info = np.iinfo(NP[tag])
    if distinct:
        return rng.integers(max(info.min, -distinct), min(info.max, distinct) + 1, n).astype(NP[tag])
    return rng.integers(info.min, info.max, n, dtype=NP[tag], endpoint=True)


ALL_TAGS = [INT8, INT16, INT32, INT64, INT128, UINT8, UINT16, UINT32, UINT64, UINT128, BOOL, FLOAT, DOUBLE]


@pytest.mark.parametrize("tag", ALL_TAGS)
def test_every_dtype_asc_desc_every_size(dev, tag):
    rng = np.random.default_rng(tag)
    for n in SIZES:
        for distinct in (None, 50):
            x = rand_col(rng, tag, n, distinct)
            for o in (ORDER_ASC, ORDER_DESC):
                got = dev.sort_rows(tagged(dev, [x]), [o])
                assert np.array_equal(got, want_order([x], [o])), (tag, n, distinct, o)


@pytest.mark.parametrize("tag", [UINT32, UINT64, UINT128, INT32, INT64, UINT8])
def test_neg_is_ascending_negation_in_the_key_width(dev, tag):
    rng = np.random.default_rng(100 + tag)
    for n in (1, 65, SMALL + 1, 300_000):
        x = rand_col(rng, tag, n, 40)
        if tag in (UINT32, UINT64):
            x[: n // 3] = 0
            neg = np.zeros(1, x.dtype) - x                                  # (-x) mod 2^w (unsigned wrap), stable order over it
            want = np.argsort(neg, kind="stable").astype(np.uint32)
            assert np.array_equal(want, want_order([x], [ORDER_NEG]))
        got = dev.sort_rows([x], [ORDER_NEG])
        assert np.array_equal(got, want_order([x], [ORDER_NEG])), (tag, n)
    x = np.array([5, 0, 1, 0, 2**32 - 1, 7], dtype=np.uint32)
    assert list(dev.sort_rows([x], [ORDER_NEG])) == [1, 3, 4, 5, 0, 2]


def test_mixed_keys_with_heavy_ties(dev):
    rng = np.random.default_rng(7)
    shapes = [
        ([INT32, INT32], [ORDER_ASC, ORDER_DESC]),
        ([INT64, UINT32, DOUBLE], [ORDER_DESC, ORDER_NEG, ORDER_ASC]),
        ([UINT8, INT16, FLOAT, INT64], [ORDER_ASC, ORDER_DESC, ORDER_DESC, ORDER_ASC]),
        ([BOOL, INT128, UINT16], [ORDER_DESC, ORDER_ASC, ORDER_ASC]),
        ([DOUBLE, UINT128], [ORDER_ASC, ORDER_NEG]),
        ([INT8, INT8, INT8, INT8], [ORDER_ASC, ORDER_DESC, ORDER_ASC, ORDER_DESC]),
    ]
    for n in (63, SMALL, SMALL + 1, CHUNK + 1, 1_000_003):
        for tags, orders in shapes:
            keys = [rand_col(rng, t, n, 3) for t in tags]
            got = dev.sort_rows(tagged(dev, keys), orders)
            assert np.array_equal(got, want_order(keys, orders)), (n, tags, orders)


def test_float_specials_and_integer_extremes(dev):
    rng = np.random.default_rng(11)
    specials = [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1.0, -1.0, 5e-324, -5e-324]
    for n in (40, SMALL + 7, 200_000):
        for tag in (FLOAT, DOUBLE):
            x = np.array(rng.choice(np.array(specials, dtype=np.float64), n), dtype=NP[tag])
            if tag == FLOAT:                                # other NaN payloads, either sign
                x.view(np.uint32)[::7] = 0xFF80BEEF
            else:
                x.view(np.uint64)[::7] = 0x7FF00000DEADBEEF
            tie = rng.integers(0, 3, n).astype(np.int32)
            for o in (ORDER_ASC, ORDER_DESC):
                got = dev.sort_rows([x], [o])
                assert np.array_equal(got, want_order([x], [o])), (tag, n, o)
                got = dev.sort_rows([x, tie], [o, ORDER_DESC])
                assert np.array_equal(got, want_order([x, tie], [o, ORDER_DESC])), (tag, n, o)
                s = x[got]
                fin = s[~np.isnan(s)]
                assert np.all(fin[1:] >= fin[:-1]) if o == ORDER_ASC else np.all(fin[1:] <= fin[:-1])
                nan_at = np.flatnonzero(np.isnan(s))
                if o == ORDER_ASC:
                    assert np.array_equal(nan_at, np.arange(len(s) - len(nan_at), len(s)))
                else:
                    assert np.array_equal(nan_at, np.arange(len(nan_at)))
        for tag in (INT32, UINT32, INT64, UINT64, INT128, UINT128):
            if tag in (INT128, UINT128):
                x = rand_col(rng, tag, n, 2)
                ext = np.zeros(4, dtype=NP[tag])
                ext["lo"] = [0, 2**64 - 1, 0, 2**64 - 1]
                ext["hi"] = [-2**63, 2**63 - 1, 0, -1] if tag == INT128 else np.array([0, 2**64 - 1, 0, 1], dtype=np.uint64)
            else:
                info = np.iinfo(NP[tag])
                x = rand_col(rng, tag, n, 5)
                ext = np.array([info.min, info.max, 0, info.max - 1], dtype=NP[tag])
            x[rng.integers(0, n, n // 2)] = ext[rng.integers(0, 4, n // 2)]
            for o in (ORDER_ASC, ORDER_DESC) + ((ORDER_NEG,) if tag in (UINT32, UINT64, UINT128) else ()):
                got = dev.sort_rows([x], [o])
                assert np.array_equal(got, want_order([x], [o])), (tag, n, o)


def test_rows_in_subset_with_repeats_and_in_place(dev):
    rng = np.random.default_rng(13)
    for n in (100, SMALL + 3, 700_001):
        a = rand_col(rng, INT64, n, 1000)
        b = rand_col(rng, FLOAT, n, 10)
        for m in (1, 50, SMALL - 1, SMALL + 1, 2 * n):
            rows = rng.integers(0, n, m).astype(np.uint32)
            got = dev.sort_rows([a, b], [ORDER_ASC, ORDER_DESC], rows=rows)
            assert np.array_equal(got, want_order([a, b], [ORDER_ASC, ORDER_DESC], rows)), (n, m)
            buf = dev.to_device(rows)                   # rows_out == rows_in
            dev.sort_rows([a, b], [ORDER_ASC, ORDER_DESC], rows=buf, out=buf, keep=True)
            assert np.array_equal(buf.to_host(), want_order([a, b], [ORDER_ASC, ORDER_DESC], rows)), (n, m)
            one = dev.to_device(rows)                   # in place with one pass
            dev.sort_rows([a % 200], [ORDER_ASC], rows=one, out=one, keep=True)
            assert np.array_equal(one.to_host(), want_order([a % 200], [ORDER_ASC], rows)), (n, m)


def test_rows_out_overlapping_rows_in(dev):
    """rows_out half over rows_in, for a constant key (no pass runs: the input order is copied) and for a varying one"""
    rng = np.random.default_rng(23)
    n = 300_000
    for key in (np.full(n, 3, np.int32), rng.integers(0, 1000, n).astype(np.int32)):
        rows = rng.integers(0, n, n).astype(np.uint32)
        big = dev.to_device(np.concatenate([rows, np.zeros(n // 2, np.uint32)]))
        rin = DevBuf(dev, big.ptr, np.uint32, n, owned=False)
        rout = DevBuf(dev, big.ptr + 4 * (n // 2), np.uint32, n, owned=False)
        dev.sort_rows([key], [ORDER_ASC], rows=rin, out=rout, keep=True)
        assert np.array_equal(rout.to_host(), want_order([key], [ORDER_ASC], rows))
        big.free()


def test_pass_skipping(dev):
    rng = np.random.default_rng(17)
    for n in (SMALL, 1_000_003):
        ids = rng.integers(1, 101, n).astype(np.int64)
        got = dev.sort_rows([ids], [ORDER_ASC])
        assert dev.sort_last_passes() == 1
        assert np.array_equal(got, want_order([ids], [ORDER_ASC]))
        const = np.full(n, 12345, dtype=np.int64)
        got = dev.sort_rows([const], [ORDER_DESC])
        assert dev.sort_last_passes() == 0
        assert np.array_equal(got, np.arange(n, dtype=np.uint32))
        rows = rng.integers(0, n, n // 3).astype(np.uint32)
        assert np.array_equal(dev.sort_rows([const], [ORDER_ASC], rows=rows), rows)
        t = rng.integers(0, 10_000, n).astype(np.int32)
        got = dev.sort_rows([t], [ORDER_ASC])
        assert dev.sort_last_passes() == 2
        assert np.array_equal(got, want_order([t], [ORDER_ASC]))
        u = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        got = dev.sort_rows([u], [ORDER_ASC])
        assert dev.sort_last_passes() == 4
        assert np.array_equal(got, want_order([u], [ORDER_ASC]))


def test_1e8_random_uint32_is_a_sorted_permutation(dev):
    n = 100_000_000
    x = np.random.default_rng(19).integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    got = dev.sort_rows([x], [ORDER_ASC])
    assert got.shape == (n,)
    assert np.all(np.bincount(got, minlength=n) == 1)
    s = x[got]
    assert np.all(s[1:] >= s[:-1])


def test_error_codes_leave_the_output_untouched(dev):
    x = np.arange(10, dtype=np.float64)
    sentinel = np.full(10, 0xDEADBEEF, dtype=np.uint32)
    codes = dev.to_device(np.arange(10, dtype=np.uint32))     # a STR column's dictionary codes, tagged STR
    codes._tag = STR
    cases = [
        (lambda out: dev.sort_rows([codes], [ORDER_ASC], out=out, keep=True), 2),
        (lambda out: dev.sort_rows([], [], rows=np.arange(10, dtype=np.uint32), out=out, keep=True), 3),
        (lambda out: dev.sort_rows([x], [ORDER_NEG], out=out, keep=True), 3),
        (lambda out: dev.sort_rows([x], [7], out=out, keep=True), 3),
    ]
    for call, code in cases:
        out = dev.to_device(sentinel)
        with pytest.raises(AqgError) as e:
            call(out)
        assert e.value.code == code
        assert np.array_equal(out.to_host(), sentinel)
