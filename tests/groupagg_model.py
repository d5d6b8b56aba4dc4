"""The plain-Python model of ONE group's aggregate (include/aqg.h: aqg_groupby_agg, aqg_grouped_reduce).

It does not come from oracle/aq_oracle.c: it is written from the reference's formulas and the C++ rules, in python `int` and python
`float`, so that it is a second opinion on the oracle the GPU tests are held to (tests/test_groupagg_model.py holds the oracle to it).

  integers   sum: exact, in python int (it always fits the 128-bit result type).  min / max: the sequential fold from the reference's
             seeds, max() for min and numeric_limits<T>::min() for max.  count: the number of rows.  avg: float(sum) / n -- one
             rounding of the exact sum, one division.  var: (ssq - s * s / (n + 1)) / (n + 1) with every product x * x evaluated
             in the PROMOTED type of the column (int for 1- and 2-byte columns; it wraps, and the wrapped value -- negative for some
             uint16 rows -- is what the 128-bit sum of squares takes), s * s wrapped in the 128-bit result type (signed for signed
             columns, unsigned for unsigned ones), both converted to double by one rounding.  stddev: sqrt(var).
  floating   min / max: the same fold, compared with `<` / `>` like the reference (a NaN row makes it forget what came before).
             sum / avg / var are not modelled bit for bit -- any summation order is allowed within a bound -- so the model gives
             what the bound is made of: the exact sum of the finite rows (math.fsum), sum |x| and sum x^2 over them.
"""
import math

import numpy as np


def _wrap(v, signed, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if signed and v >> (bits - 1) else v


def promoted(dt):
    """(signed, bits) of the type `x * x` is evaluated in: integer promotion [conv.prom]"""
    dt = np.dtype(dt)
    assert dt.kind in "iu"
    if dt.itemsize < 4:
        return True, 32
    return dt.kind == "i", dt.itemsize * 8


def seeds(dt):
    """(seed of min, seed of max): numeric_limits<T>::max() and numeric_limits<T>::min() -- for floating types the latter is the
    smallest positive normal value"""
    dt = np.dtype(dt)
    if dt.kind == "f":
        fi = np.finfo(dt)
        return float(fi.max), float(fi.tiny)
    ii = np.iinfo(dt)
    return int(ii.max), int(ii.min)


def fold_min(values, dt):
    m = seeds(dt)[0]
    for v in values:
        m = m if m < v else v
    return m


def fold_max(values, dt):
    m = seeds(dt)[1]
    for v in values:
        m = m if m > v else v
    return m


def int_sum(values):
    return sum(values)


def int_avg(values):
    return float(sum(values)) / float(len(values))


def int_var(values, dt):
    """(ssq - s * s / (double)(n + 1)) / (double)(n + 1), the two sums in the 128-bit result type of the column"""
    signed, bits = promoted(dt)
    long_signed = np.dtype(dt).kind == "i"
    s = _wrap(sum(values), long_signed, 128)
    ssq = _wrap(sum(_wrap(v * v, signed, bits) for v in values), long_signed, 128)
    ss = _wrap(s * s, long_signed, 128)
    np1 = float((len(values) + 1) & 0xFFFFFFFF)
    return (float(ssq) - float(ss) / np1) / np1


def int_stddev(values, dt):
    v = int_var(values, dt)
    return math.sqrt(v) if v >= 0 else math.nan


def int_group(values, dt):
    """every modelled aggregate of one group of an integer column; `values`: python ints in row order"""
    return dict(sum=int_sum(values), min=fold_min(values, dt), max=fold_max(values, dt), count=len(values), avg=int_avg(values),
                var=int_var(values, dt), stddev=int_stddev(values, dt))


def fp_group(values, dt):
    """one group of a floating column; `values`: python floats in row order (a float32 value is exact as a python float).
    min / max bit for bit; for the sums: n, whether a row is NaN / +Inf / -Inf, and over the FINITE rows the exact sum, sum |x| and
    sum x^2 (the last two rounded up by at most a few ulp: they only size a bound)"""
    fin = [v for v in values if math.isfinite(v)]
    return dict(min=fold_min(values, dt), max=fold_max(values, dt), count=len(values), nan=any(v != v for v in values),
                pinf=any(v == math.inf for v in values), ninf=any(v == -math.inf for v in values),
                exact_sum=_fsum(fin), sum_abs=_fsum(abs(v) for v in fin), sum_sq=_fsum(v * v for v in fin))


def _fsum(it):
    try:
        return math.fsum(it)
    except OverflowError:                                   # (partial sums beyond the double range: such a column sizes no finite bound)
        return math.inf
