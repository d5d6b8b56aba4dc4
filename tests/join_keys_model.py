"""The model of the joins on composite and typed keys (include/aqg.h: aqg_join_keys_count / _pairs / _lookup).

The reference runs its joins in MonetDB, so the contract is the library's own and this file states it in plain Python: every row of
a side becomes a canonical tuple, a dict maps each build tuple to its ascending rows, and the four kinds read that dict.
A side is a list of (tag, data) columns in the format of tests/keycases.py: numpy arrays for integers, bool, floating and 128-bit
columns (checker.I128 / U128), (n, bytes) uint8 arrays for DATE / TIME / TIMESTAMP, lists of bytes objects for strings (the
library joins those through the codes of ONE dictionary over both sides: content equality).  Equality, column by column:
    integers, bool   by value (Python ints)
    DATE             its 4 bytes;   TIME  its 7 field bytes (the 8th is padding);   TIMESTAMP  date plus time
    128-bit          (hi, lo)
    floating         by ==: -0.0 -> 0.0, and a row holding a NaN in any key column matches nothing (its tuple is None)
No C behind it; tests/test_join_keys_model.py holds it to tests/join_model.py, to nested loops and to the real reference's
grouping (tests/golden/ref_golden_keys.json)."""
import math

import numpy as np

import checker as ck

NONE = 0xFFFFFFFF
INNER, LEFT, SEMI, ANTI = range(4)


def _column(tag, data):
    """the canonical values of one column, a list of n hashable values (None for a NaN)"""
    if tag == ck.STR:
        return [bytes(s) for s in data]
    a = np.asarray(data)
    if tag == ck.DATE:
        return [bytes(r) for r in a.reshape(len(a), -1)[:, :4]]
    if tag == ck.TIME:
        return [bytes(r) for r in a.reshape(len(a), -1)[:, :7]]
    if tag == ck.TIMESTAMP:
        return [bytes(r) for r in a.reshape(len(a), -1)[:, :11]]
    if a.dtype.names:                                            # 128-bit: (hi, lo)
        return list(zip(a["hi"].tolist(), a["lo"].tolist()))
    if a.dtype.kind == "f":
        return [None if math.isnan(v) else v + 0.0 for v in a.astype(np.float64).tolist()]      # -0.0 + 0.0 == +0.0; float32 -> float64 is exact
    if a.dtype.kind == "b":
        return a.astype(np.uint8).tolist()
    assert a.dtype.kind in "iu", a.dtype
    return a.tolist()


def rows(cols):
    """the canonical tuple of every row of a side, None for a row that matches nothing"""
    vals = [_column(tag, data) for tag, data in cols]
    return [None if any(v is None for v in t) else t for t in zip(*vals)]


def _table(build):
    table = {}
    for r, t in enumerate(rows(build)):
        if t is not None:
            table.setdefault(t, []).append(r)                    # ascending build rows
    return table


def distinct(build):
    """(G, table slots): the distinct tuples of the build side as aqg_groupby_build counts them -- every NaN row a group of its own --
    and the power of two >= 2G, at least 16"""
    r = rows(build)
    G = len({t for t in r if t is not None}) + sum(t is None for t in r)
    slots = 16
    while slots < 2 * G:
        slots *= 2
    return G, slots


def matches(build, probe):
    """for every probe row the list of its build rows, ascending (empty: no partner)"""
    table = _table(build)
    return [table.get(t, []) if t is not None else [] for t in rows(probe)]


def pairs(kind, build, probe, m=None):
    """(probe_rows, build_rows) as uint32 arrays; build_rows is None for SEMI / ANTI.  m: matches(build, probe), where a caller
    asks several questions about one pair of sides"""
    m = matches(build, probe) if m is None else m
    if kind == SEMI:
        return np.array([i for i, b in enumerate(m) if b], dtype=np.uint32), None
    if kind == ANTI:
        return np.array([i for i, b in enumerate(m) if not b], dtype=np.uint32), None
    assert kind in (INNER, LEFT)
    pr, br = [], []
    for i, b in enumerate(m):
        if not b and kind == LEFT:
            b = [NONE]
        pr += [i] * len(b)
        br += b
    return np.array(pr, dtype=np.uint32), np.array(br, dtype=np.uint32)


def count(kind, build, probe, m=None):
    """the number of output rows, a Python int (exact beyond 2^64)"""
    if m is None:
        table = {t: len(r) for t, r in _table(build).items()}
        c = [table.get(t, 0) if t is not None else 0 for t in rows(probe)]
    else:
        c = [len(b) for b in m]
    if kind == INNER:
        return sum(c)
    if kind == LEFT:
        return sum(max(x, 1) for x in c)
    if kind == SEMI:
        return sum(x > 0 for x in c)
    assert kind == ANTI
    return sum(x == 0 for x in c)


def lookup(build, probe, m=None):
    """uint32[np]: the LOWEST build row whose tuple equals probe row i, else 0xFFFFFFFF"""
    m = matches(build, probe) if m is None else m
    return np.array([b[0] if b else NONE for b in m], dtype=np.uint32)
