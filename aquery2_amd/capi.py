"""ctypes binding of the C-ABI (include/aqg.h).  Test/bench harness only: numpy in, numpy out.

There is NO fallback: if libaqg.so is missing or no GPU is visible, construction raises.
"""
import ctypes as C
import os
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# dtype tags (reference server/aquery_types.h:1-5)
INT32, FLOAT, STR, DOUBLE, LDOUBLE, INT64, INT128, INT16, DATE, TIME, INT8 = range(11)
UINT32, UINT64, UINT128, UINT16, UINT8, BOOL = 11, 12, 13, 14, 15, 16
TIMESTAMP = 18
ERROR = 22
I128 = np.dtype([("lo", "<u8"), ("hi", "<i8")])
U128 = np.dtype([("lo", "<u8"), ("hi", "<u8")])
TAG2NP = {
    INT8: np.dtype(np.int8), INT16: np.dtype(np.int16), INT32: np.dtype(np.int32), INT64: np.dtype(np.int64),
    UINT8: np.dtype(np.uint8), UINT16: np.dtype(np.uint16), UINT32: np.dtype(np.uint32), UINT64: np.dtype(np.uint64),
    FLOAT: np.dtype(np.float32), DOUBLE: np.dtype(np.float64), BOOL: np.dtype(np.uint8), INT128: I128, UINT128: U128,
}
NP2TAG = {v: k for k, v in TAG2NP.items() if k != BOOL}
NP2TAG[np.dtype(np.bool_)] = BOOL
VEC_VEC, VEC_SCALAR, SCALAR_VEC = 0, 1, 2
LAYOUT_ROW, LAYOUT_FLAT = 0, 1                                 # aqg_grouped_ewise: the layout of the column operand
ORDER_ASC, ORDER_DESC, ORDER_NEG = 0, 1, 2
SEL_LOWER, SEL_UPPER = 0, 1                                   # aqg_median: rank (c-1)/2 resp. c/2 of the c rows in ascending order
ROUTE_SMALL, ROUTE_GROUP, ROUTE_SPLIT = 1, 2, 4               # aqg_select_last_routes
# ctypes prototypes of the median entries (applied by load_library)
MEDIAN_PROTOTYPES = {
    "aqg_median": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p],
    "aqg_grouped_median": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "aqg_grouped_median_flat": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "aqg_select_last_routes": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
}
# ctypes prototypes of the top-k entries (applied by load_library)
TOPK_MAX = 1024
TOPK_PROTOTYPES = {
    "aqg_topk": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p],
    "aqg_grouped_topk": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "aqg_grouped_topk_flat": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
}
# ctypes prototypes of the quantile entries (applied by load_library)
QUANTILES_MAX = 8
QUANTILE_PROTOTYPES = {
    "aqg_quantiles": [C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p],
    "aqg_grouped_quantiles": [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_int, C.c_void_p, C.c_void_p],
    "aqg_grouped_quantiles_flat": [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_int, C.c_void_p, C.c_void_p],
}
# ctypes prototypes of the moving-quantile entries (applied by load_library)
WINQ_MAX_W = 1024
WINQ_PROTOTYPES = {
    "aqg_window_quantiles": [C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
    "aqg_grouped_window_quantiles": [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p],
    "aqg_grouped_window_quantiles_flat": [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p],
    "aqg_window_quantiles_last": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
}
# ctypes prototypes of the ranking entries (applied by load_library); RANK_*: aqg_rank's methods, RANK_ROUTE_*: aqg_rank_last
RANK_MIN, RANK_MAX, RANK_DENSE, RANK_FIRST, RANK_AVERAGE, RANK_PERCENT, RANK_CUME_DIST, RANK_NTILE = range(8)
RANK_ROUTE_SMALL, RANK_ROUTE_SORTED = 1, 2
RANK_PROTOTYPES = {
    "aqg_rank_out_dtype": [C.c_int],
    "aqg_rank": [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p],
    "aqg_grouped_rank": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p],
    "aqg_grouped_rank_flat": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p],
    "aqg_rank_last": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
}
# ctypes prototypes of the pair windows (applied by load_library); SCAN2_*: aqg_scan2's ops, SCAN2_ROUTE_*: aqg_scan2_last
SCAN2_COVS, SCAN2_CORRS, SCAN2_BETAS, SCAN2_COVW, SCAN2_CORRW, SCAN2_BETAW = range(6)
SCAN2_ROUTE_REG, SCAN2_ROUTE_LDS, SCAN2_ROUTE_PREFIX = 1, 2, 4
SCAN2_PROTOTYPES = {
    "aqg_scan2": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
    "aqg_grouped_scan2": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p],
    "aqg_grouped_scan2_flat": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p],
    "aqg_scan2_last": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
}
# ctypes prototypes of the exponential moving averages (applied by load_library)
EMA_RECURSIVE, EMA_ADJUSTED = 0, 1
EMA_PROTOTYPES = {
    "aqg_scan_ema": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p],
    "aqg_grouped_ema": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p],
    "aqg_grouped_ema_flat": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p],
    "aqg_decay_from_times": [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p],
    "aqg_grouped_decay_from_times_flat": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_void_p],
}
# ctypes prototypes of the time-range windows (applied by load_library)
RANGEW_COUNT, RANGEW_SUM, RANGEW_AVG, RANGEW_MIN, RANGEW_MAX = range(5)
RANGEW_OPEN, RANGEW_CLOSED = 0, 1
RANGEW_PROTOTYPES = {
    "aqg_rangew_out_dtype": [C.c_int, C.c_int],
    "aqg_rangew_bounds": [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_double, C.c_int, C.c_void_p],
    "aqg_grouped_rangew_bounds_flat": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_void_p],
    "aqg_rangew_fold": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "aqg_rangew": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p],
    "aqg_grouped_rangew": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "aqg_grouped_rangew_flat": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "aqg_rangew_last": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
}
# ctypes prototypes of the count-distinct entries (applied by load_library)
DISTINCT_PROTOTYPES = {
    "aqg_count_distinct": [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)],
    "aqg_grouped_count_distinct": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "aqg_grouped_count_distinct_flat": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "aqg_distinct_last": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)],
}
# ctypes prototypes of the joins on composite and typed keys (applied by load_library)
JOIN_INNER, JOIN_LEFT, JOIN_SEMI, JOIN_ANTI = range(4)
JOIN_ROUTE_PACKED, JOIN_ROUTE_WIDE, JOIN_ROUTE_LDS, JOIN_ROUTE_HBM = 1, 2, 4, 8          # aqg_join_last
JOIN_KEYS_PROTOTYPES = {
    "aqg_join_keys_count": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)],
    "aqg_join_keys_pairs": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                            C.c_uint64, C.POINTER(C.c_uint64)],
    "aqg_join_keys_lookup": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p],
    "aqg_join_last": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
    "aqg_join_tuple_slots": [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
    "aqg_gather_fill": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
}
# ctypes prototypes of the as-of join (applied by load_library)
ASOF_BACKWARD, ASOF_FORWARD = 0, 1
ASOF_STRICT = 1                                                                        # flags
ASOF_ROUTE_LDS, ASOF_ROUTE_HBM, ASOF_ROUTE_NOKEYS, ASOF_ROUTE_PRESORTED = 1, 2, 4, 8    # aqg_join_asof_last
ASOF_PROTOTYPES = {
    "aqg_join_asof": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                      C.c_int, C.c_void_p],
    "aqg_join_asof_last": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
}
# ctypes prototypes of the window join (applied by load_library)
WJ_OPEN_LO, WJ_OPEN_HI, WJ_PREVAILING = 1, 2, 4                                         # flags
WJ_FOLD_STAGED, WJ_FOLD_INPLACE = 16, 32                                                # aqg_join_window_last, beside the ASOF_ROUTE_* bits
WJ_PROTOTYPES = {
    "aqg_join_window_bounds": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                               C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p],
    "aqg_interval_fold": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "aqg_join_window": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                        C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "aqg_join_window_last": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
}
STR_ROUTE_HOST, STR_ROUTE_DEVICE, STR_ROUTE_FALLBACK = 1, 2, 4                          # aqg_str_encode_last
STR_PROTOTYPES = {
    "aqg_str_encode_last": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
}
# the scratch-memory guard (test aids of include/aqg.h; on in a process started with AQG_WS_GUARD=<byte>)
WS_CLEAN, WS_ZONE, WS_PADDING, WS_TAIL, WS_RANK_BM = range(5)


class WsReport(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("alloc_index", C.c_int32), ("offset", C.c_uint64), ("alloc_offset", C.c_uint64),
                ("alloc_bytes", C.c_uint64), ("expected", C.c_uint8), ("found", C.c_uint8), ("pad_", C.c_uint8 * 6)]


class WsInfo(C.Structure):
    _fields_ = [("base", C.c_void_p), ("physical_bytes", C.c_uint64), ("logical_bytes", C.c_uint64), ("rank_bm", C.c_void_p),
                ("rank_bm_bytes", C.c_uint64), ("nallocs", C.c_uint32), ("guard", C.c_uint8), ("pattern", C.c_uint8), ("pad_", C.c_uint8 * 2)]


DEBUG_PROTOTYPES = {
    "aqg_debug_ws_check": [C.c_void_p, C.POINTER(WsReport)],
    "aqg_debug_ws_info": [C.c_void_p, C.POINTER(WsInfo), C.c_void_p, C.c_uint32],
}
PLAN_FAST_LDS, PLAN_SMALL_LDS, PLAN_BIG_LDS, PLAN_DENSE, PLAN_PART_ONE, PLAN_PART_TWO, PLAN_PART_ROUND1, PLAN_PART_WIDE, PLAN_SORTED_TAIL, PLAN_HBM_TABLE, PLAN_BUILD_PARTITIONED, PLAN_GID_PARTITION, PLAN_PACKED_VALUES, PLAN_RANGE_PARTITIONS, PLAN_ROW_EMIT, PLAN_PACKED_KEYS, PLAN_BUILD_LOOKUP = (1 << i for i in range(17))


class AqgError(RuntimeError):
    def __init__(self, what, code, detail=""):
        super().__init__(f"{what}: status {code} {detail}")
        self.code = code


def lib_path():
    return os.path.join(HERE, "libaqg.so")


_LIB = None


def load_library():
    """dlopen the in-tree libaqg.so; raises if it has not been built (no fallback)."""
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise FileNotFoundError(f"{p} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                    "or `make -C aquery2_amd/csrc`")
        lib = C.CDLL(p)
        lib.aqg_version.restype = C.c_char_p
        lib.aqg_last_error.restype = C.c_char_p
        lib.aqg_dtype_size.restype = C.c_size_t
        lib.aqg_ctx_stream.restype = C.c_void_p
        lib.aqg_groupby_ngroups.restype = C.c_uint32
        lib.aqg_groupby_nrows.restype = C.c_uint32
        lib.aqg_groupby_first_rows64.restype = C.c_void_p
        for f in ("aqg_groupby_reversemap", "aqg_groupby_counts", "aqg_groupby_first_rows", "aqg_groupby_agg_result"):
            getattr(lib, f).restype = C.c_void_p
        for f, argtypes in list(MEDIAN_PROTOTYPES.items()) + list(TOPK_PROTOTYPES.items()) + list(QUANTILE_PROTOTYPES.items()) + list(WINQ_PROTOTYPES.items()) + list(RANK_PROTOTYPES.items()) + list(SCAN2_PROTOTYPES.items()) + list(EMA_PROTOTYPES.items()) + list(RANGEW_PROTOTYPES.items()) + list(DISTINCT_PROTOTYPES.items()) + list(JOIN_KEYS_PROTOTYPES.items()) + list(STR_PROTOTYPES.items()) + list(ASOF_PROTOTYPES.items()) + list(WJ_PROTOTYPES.items()) + list(DEBUG_PROTOTYPES.items()):
            getattr(lib, f).argtypes, getattr(lib, f).restype = argtypes, C.c_int
        _LIB = lib
    return _LIB


def tag_of(a):
    return NP2TAG[np.asarray(a).dtype]


def join_tuple_slots(cols, table_slots):
    """aqg_join_tuple_slots (host code, no GPU): the first slot the join kernels try for every tuple of the HOST key columns `cols`
    -- numpy arrays, or (tag, array) pairs for DATE / TIME / TIMESTAMP columns given as (n, bytes) uint8 arrays -- in a table of
    `table_slots` slots"""
    lib = load_library()
    pairs = [c if isinstance(c, tuple) else (tag_of(c), c) for c in cols]
    arrs = [np.ascontiguousarray(a.astype(np.uint8) if np.asarray(a).dtype == np.bool_ else a) for _, a in pairs]
    n = len(arrs[0]) if arrs else 0
    dts = (C.c_int * max(1, len(pairs)))(*[t for t, _ in pairs])
    ptrs = (C.c_void_p * max(1, len(pairs)))(*[a.ctypes.data for a in arrs])
    out = np.empty(n, np.uint32)
    rc = lib.aqg_join_tuple_slots(len(pairs), dts, ptrs, n, int(table_slots), out.ctypes.data)
    if rc != 0:
        raise AqgError("aqg_join_tuple_slots", rc)
    return out


class DevBuf:
    """A device allocation (HBM) with a dtype and element count."""

    def __init__(self, dev, ptr, dtype, n, owned=True):
        self.dev, self.ptr, self.dtype, self.n, self.owned = dev, ptr, np.dtype(dtype), int(n), owned

    @property
    def tag(self):
        if getattr(self, "_tag", None) is not None:
            return self._tag
        return NP2TAG[self.dtype] if self.dtype in NP2TAG else (INT128 if self.dtype == I128 else UINT128)

    @property
    def __cuda_array_interface__(self):
        """zero-copy view for torch.as_tensor(buf, device="cuda") (bench.py's RCCL merge); 128-bit
        columns are exposed as 2n int64 words"""
        if self.dtype.names:
            return {"shape": (2 * self.n,), "typestr": "<i8", "data": (int(self.ptr), False), "version": 3}
        return {"shape": (self.n,), "typestr": self.dtype.str, "data": (int(self.ptr), False), "version": 3}

    def to_host(self):
        out = np.empty(self.n, dtype=self.dtype)
        if self.n:
            self.dev._chk(self.dev.lib.aqg_d2h(self.dev.ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr),
                                               C.c_size_t(out.nbytes)), "aqg_d2h")
        return out

    def free(self):
        if self.owned and self.ptr and self.dev.ctx:
            self.dev.lib.aqg_free(self.dev.ctx, C.c_void_p(self.ptr))
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class GroupBy:
    def __init__(self, dev, handle):
        self.dev, self.h = dev, handle
        dev._handles.add(self)

    @property
    def ngroups(self):
        return self.dev.lib.aqg_groupby_ngroups(self.h)

    @property
    def plan(self):
        """AQG_PLAN_* bits of the plan the last call through this handle took"""
        self.dev.lib.aqg_groupby_plan.restype = C.c_uint32
        return self.dev.lib.aqg_groupby_plan(self.h)

    def _view(self, fn, dtype, n):
        p = getattr(self.dev.lib, fn)(self.h)
        if not p:
            return None
        return DevBuf(self.dev, p, dtype, n, owned=False).to_host()

    def reversemap(self):
        return self._view("aqg_groupby_reversemap", np.uint32, self.dev.lib.aqg_groupby_nrows(self.h))

    def counts(self):
        return self._view("aqg_groupby_counts", np.uint32, self.ngroups)

    def first_rows(self):
        return self._view("aqg_groupby_first_rows", np.uint32, self.ngroups)

    def first_rows64(self):
        """global row id of every group's first row (handles of aqg_groupby_agg_sharded)"""
        return self._view("aqg_groupby_first_rows64", np.int64, self.ngroups)

    def keys_raw(self, k, elem_bytes):
        """key column k of every group as raw bytes, (ngroups, elem_bytes) uint8 (keys of any element type)"""
        out = self.dev.empty(max(1, self.ngroups * elem_bytes), np.uint8)
        self.dev._chk(self.dev.lib.aqg_groupby_keys(self.h, k, C.c_void_p(out.ptr)), "aqg_groupby_keys")
        self.dev.sync()
        return out.to_host()[:self.ngroups * elem_bytes].reshape(self.ngroups, elem_bytes)

    def keys(self, k, dtype):
        out = self.dev.empty(self.ngroups, dtype)
        self.dev._chk(self.dev.lib.aqg_groupby_keys(self.h, k, C.c_void_p(out.ptr)), "aqg_groupby_keys")
        self.dev.sync()
        return out.to_host()

    def result(self, j, op, val_tag):
        ot = self.dev.lib.aqg_reduce_out_dtype(op, val_tag)
        p = self.dev.lib.aqg_groupby_agg_result(self.h, j)
        return DevBuf(self.dev, p, TAG2NP[ot], self.ngroups, owned=False).to_host()

    def postproc(self):
        G, n = self.ngroups, self.dev.lib.aqg_groupby_nrows(self.h)
        off, rows = self.dev.empty(G + 1, np.uint32), self.dev.empty(max(n, 1), np.uint32)
        self.dev._chk(self.dev.lib.aqg_groupby_postproc(self.h, C.c_void_p(off.ptr), C.c_void_p(rows.ptr)), "aqg_groupby_postproc")
        self.dev.sync()
        return off.to_host(), rows.to_host()[:n]

    def destroy(self):
        if self.h and self.dev.ctx:
            self.dev.lib.aqg_groupby_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


class Comm:
    """One communicator of the library's own exchange (include/aqg.h: aqg_comm_*).  `nccl_id`: the AQG_COMM_ID_BYTES bytes rank 0
    got from Comm.unique_id() -- RCCL; `allgather`: a Python callable (send_ptr, recv_ptr, nbytes, stream) -> 0 -- a caller-supplied
    transport (tests / one-GPU rehearsals)."""

    def __init__(self, dev, rank, world, nccl_id=None, allgather=None):
        self.dev, self.rank, self.world = dev, rank, world
        h = C.c_void_p()
        if allgather is not None:
            self._cb = ALLGATHER_FN(lambda user, send, recv, nbytes, stream: int(allgather(send, recv, nbytes, stream)))
            dev._chk(dev.lib.aqg_comm_init_custom(dev.ctx, rank, world, self._cb, None, C.byref(h)), "aqg_comm_init_custom")
        else:
            assert nccl_id is not None and len(nccl_id) == 128
            buf = (C.c_char * 128).from_buffer_copy(bytes(nccl_id))
            dev._chk(dev.lib.aqg_comm_init_rccl(dev.ctx, rank, world, buf, C.byref(h)), "aqg_comm_init_rccl")
        self.h = h

    @staticmethod
    def unique_id(lib=None):
        lib = lib or load_library()
        buf = (C.c_char * 128)()
        rc = lib.aqg_comm_unique_id(buf)
        if rc != 0:
            raise AqgError("aqg_comm_unique_id", rc)
        return bytes(buf.raw)

    def groupby_agg_sharded(self, keys, ops, vals, row_base, hint=0, gmax=0, handle=None):
        d = self.dev
        kd, dts, ptrs = d._keyargs(keys)
        vd = [d._dev(v) if v is not None else None for v in vals]
        vdt = (C.c_int * max(1, len(vd)))(*[(v.tag if v is not None else INT32) for v in vd])
        vp = (C.c_void_p * max(1, len(vd)))(*[(v.ptr if v is not None else None) for v in vd])
        opa = (C.c_int * max(1, len(ops)))(*ops)
        h = handle.h if handle is not None else C.c_void_p()
        d._chk(d.lib.aqg_groupby_agg_sharded(self.h, len(kd), dts, ptrs, len(ops), opa, vdt, vp, C.c_uint32(kd[0].n), C.c_uint64(row_base),
                                             C.c_uint32(hint), C.c_uint32(gmax), C.byref(h)), "aqg_groupby_agg_sharded")
        gb = handle if handle is not None else GroupBy(d, h)
        gb._keep = (kd, vd)
        return gb

    def prepare_groupby_agg_sharded(self, keys, ops, vals, row_base, hint=0, gmax=0):
        """groupby_agg_sharded with its argument arrays marshalled once (Device.prepare_groupby_agg's counterpart): returns a function
        that runs the same call again on the same device columns and result handle"""
        d = self.dev
        kd, dts, ptrs = d._keyargs(keys)
        vd = [d._dev(v) if v is not None else None for v in vals]
        vdt = (C.c_int * max(1, len(vd)))(*[(v.tag if v is not None else INT32) for v in vd])
        vp = (C.c_void_p * max(1, len(vd)))(*[(v.ptr if v is not None else None) for v in vd])
        opa = (C.c_int * max(1, len(ops)))(*ops)
        h = C.c_void_p()
        args = (self.h, len(kd), dts, ptrs, len(ops), opa, vdt, vp, C.c_uint32(kd[0].n), C.c_uint64(row_base), C.c_uint32(hint), C.c_uint32(gmax), C.byref(h))
        fn, chk = d.lib.aqg_groupby_agg_sharded, d._chk
        gb = GroupBy(d, h)
        gb._keep = (kd, vd, dts, ptrs, vdt, vp, opa)

        def run():
            rc = fn(*args)
            if rc != 0:
                chk(rc, "aqg_groupby_agg_sharded")
            return gb
        return run, gb

    def str_encode_sharded(self, strs):
        """global dictionary codes of this rank's strings (list of bytes): aqg_str_encode_sharded; returns (DevBuf of uint32 codes, global distinct count)"""
        d = self.dev
        bufs = [C.create_string_buffer(b) for b in strs]
        arr = (C.c_char_p * max(1, len(bufs)))(*[C.cast(b, C.c_char_p) for b in bufs])
        out = d.empty(max(1, len(bufs)), np.uint32)
        nd = C.c_uint32()
        d._chk(d.lib.aqg_str_encode_sharded(self.h, arr, C.c_uint32(len(bufs)), C.c_void_p(out.ptr), C.byref(nd)), "aqg_str_encode_sharded")
        out.n = len(bufs)
        return out, nd.value

    def reduce_sharded(self, op, x):
        """aqg_reduce over a column sharded by row range (`x`: this rank's rows); the whole column's result on every rank"""
        d = self.dev
        xd = d._dev(x)
        buf = (C.c_ubyte * 16)()
        d._chk(d.lib.aqg_reduce_sharded(self.h, op, xd.tag, C.c_void_p(xd.ptr), C.c_uint32(xd.n), buf), "aqg_reduce_sharded")
        ot = d.lib.aqg_reduce_out_dtype(op, xd.tag)
        v = np.frombuffer(bytes(buf), dtype=TAG2NP[ot], count=1)[0]
        if ot in (INT128, UINT128):
            lo, hi = int(v["lo"]), int(v["hi"])
            return (hi << 64) + lo if ot == INT128 else (hi << 64) | lo
        return v

    def corr_sharded(self, x, y):
        d = self.dev
        xd, yd = d._dev(x), d._dev(y)
        out = C.c_double()
        d._chk(d.lib.aqg_corr_sharded(self.h, xd.tag, C.c_void_p(xd.ptr), yd.tag, C.c_void_p(yd.ptr), C.c_uint32(xd.n), C.byref(out)), "aqg_corr_sharded")
        return out.value

    def scan_sharded(self, op, x, w=0):
        d = self.dev
        xd = d._dev(x)
        ot = d.lib.aqg_scan_out_dtype(op, xd.tag)
        out = d.empty(xd.n, TAG2NP[ot])
        d._chk(d.lib.aqg_scan_sharded(self.h, op, xd.tag, C.c_void_p(xd.ptr), C.c_uint32(xd.n), C.c_uint32(w), C.c_void_p(out.ptr)), "aqg_scan_sharded")
        d.sync()
        return out.to_host()

    def groupby_exchange(self, local, merge_ops, row_base, gmax=0, handle=None):
        """the exchange alone over an existing shard table (aqg_groupby_exchange): partial p = aggregate p of `local`"""
        d = self.dev
        opa = (C.c_int * max(1, len(merge_ops)))(*merge_ops)
        h = handle.h if handle is not None else C.c_void_p()
        d._chk(d.lib.aqg_groupby_exchange(self.h, local.h, len(merge_ops), opa, C.c_uint64(row_base), C.c_uint32(gmax), C.byref(h)), "aqg_groupby_exchange")
        return handle if handle is not None else GroupBy(d, h)

    def destroy(self):
        if self.h and self.dev.ctx:
            self.dev.lib.aqg_comm_destroy(self.h)
        self.h = None


class ThreadRanks:
    """`world` ranks as THREADS of one process, each with its own context (and stream) on the same GPU, and an all-gather made of
    device copies and a barrier: drives the C code of the sharded group-by end to end where only one GPU is there (RCCL refuses two
    ranks on one device).  run(fn) calls fn(rank, dev, comm) on every rank and returns the results in rank order."""

    def __init__(self, world, device=0):
        import threading
        self.world = world
        self.devs = [Device(device) for _ in range(world)]
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world
        self.comms = [Comm(self.devs[r], r, world, allgather=self._make(r)) for r in range(world)]

    def _make(self, rank):
        def gather(send, recv, nbytes, stream):
            dev = self.devs[rank]
            dev.sync()                                   # the pack kernel behind `send` has run
            self.slots[rank] = send
            self.barrier.wait()
            for r in range(self.world):
                dev._chk(dev.lib.aqg_d2d(dev.ctx, C.c_void_p(recv + r * nbytes), C.c_void_p(self.slots[r]), C.c_size_t(nbytes)), "aqg_d2d")
            dev.sync()
            self.barrier.wait()                          # nobody reuses its send buffer before everybody has copied it
            return 0
        return gather

    def run(self, fn):
        import threading
        out, err = [None] * self.world, [None] * self.world
        def body(r):
            try:
                out[r] = fn(r, self.devs[r], self.comms[r])
            except BaseException as e:                   # noqa: BLE001 -- reported to the caller below
                err[r] = e
                self.barrier.abort()
        th = [threading.Thread(target=body, args=(r,)) for r in range(self.world)]
        for t in th: t.start()
        for t in th: t.join()
        for e in err:
            if e is not None and not isinstance(e, __import__("threading").BrokenBarrierError):
                raise e
        for e in err:
            if e is not None:
                raise e
        return out

    def close(self):
        for c in self.comms: c.destroy()
        for d in self.devs: d.close()


class Device:
    """One aqg context on one GPU.  numpy-level wrappers upload, run the HIP path, download."""

    def __init__(self, device=0, stream=None):
        self.lib = load_library()
        ctx = C.c_void_p()
        rc = self.lib.aqg_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(ctx))
        if rc != 0:
            raise AqgError("aqg_ctx_create (no MI355X visible? the HIP path has no CPU fallback)", rc)
        self.ctx = ctx
        self.stream = int(stream) if stream else 0    # 0: the library made its own stream
        self._handles = weakref.WeakSet()

    def close(self):
        if self.ctx:
            for h in list(self._handles):   # handles hold device memory of this context: release them first
                h.destroy()
            self.lib.aqg_ctx_destroy(self.ctx)
            self.ctx = None

    def _chk(self, rc, what):
        if rc != 0:
            raise AqgError(what, rc, self.lib.aqg_last_error(self.ctx).decode())

    def sync(self):
        self._chk(self.lib.aqg_sync(self.ctx), "aqg_sync")

    # -- memory
    def empty(self, n, dtype):
        dtype = np.dtype(dtype)
        p = C.c_void_p()
        self._chk(self.lib.aqg_malloc(self.ctx, C.c_size_t(max(int(n), 1) * dtype.itemsize + 64), C.byref(p)), "aqg_malloc")
        return DevBuf(self, p.value, dtype, n)

    def to_device(self, a):
        a = np.ascontiguousarray(a)
        if a.dtype == np.bool_:
            a = a.astype(np.uint8)
        b = self.empty(a.size, a.dtype)
        if a.size:
            self._chk(self.lib.aqg_h2d(self.ctx, C.c_void_p(b.ptr), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes)), "aqg_h2d")
        return b

    def _dev(self, a):
        return a if isinstance(a, DevBuf) else self.to_device(a)

    def key_col(self, tag, data):
        """a key column of a type that is not a numpy scalar type: DATE / TIME / TIMESTAMP as an (n, bytes) uint8 array, FLOAT /
        DOUBLE / 128-bit columns as their arrays, STR as a list of bytes objects (encoded to uint32 codes by aqg_str_encode)"""
        if tag == STR:
            bufs = [C.create_string_buffer(b) for b in data]
            arr = (C.c_char_p * max(1, len(bufs)))(*[C.cast(b, C.c_char_p) for b in bufs])
            out = self.empty(max(1, len(bufs)), np.uint32)
            nd = C.c_uint32()
            self._chk(self.lib.aqg_str_encode(self.ctx, arr, C.c_uint32(len(bufs)), C.c_void_p(out.ptr), C.byref(nd)), "aqg_str_encode")
            out.n = len(bufs)
            out.ndistinct = nd.value
            return out
        a = np.ascontiguousarray(data)
        raw = self.to_device(a.reshape(-1).view(np.uint8))
        buf = DevBuf(self, raw.ptr, np.uint8, a.shape[0], owned=False)
        buf._raw, buf._tag = raw, tag
        return buf

    def str_encode_last(self):
        """(STR_ROUTE_* of the last aqg_str_encode on this device, 1 if its verify kernel saw a mismatch else 0)"""
        r, m = C.c_uint32(), C.c_uint32()
        self._chk(self.lib.aqg_str_encode_last(self.ctx, C.byref(r), C.byref(m)), "aqg_str_encode_last")
        return r.value, m.value

    # -- generators
    def col_pin(self, a):
        """device mirror of a borrowed host column (aqg_col_pin: asynchronous, stream-ordered upload); `a` must stay alive"""
        assert a.flags["C_CONTIGUOUS"]
        d = C.c_void_p()
        self._chk(self.lib.aqg_col_pin(self.ctx, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), C.byref(d)), "aqg_col_pin")
        buf = DevBuf(self, d.value, a.dtype, a.size, owned=False)
        buf._host = a
        return buf

    def col_pin_last(self):
        """(registered, staged, pageable) chunk counts of the most recent col_pin upload"""
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self.lib.aqg_col_pin_last(self.ctx, C.byref(a), C.byref(b), C.byref(c)), "aqg_col_pin_last")
        return a.value, b.value, c.value

    def col_unpin_all(self):
        self._chk(self.lib.aqg_col_unpin_all(self.ctx), "aqg_col_unpin_all")

    def gen_column(self, col, seed, row_base, n, n_total, K, out=None):
        dt = np.float32 if col == 8 else np.int32
        out = out or self.empty(n, dt)
        self._chk(self.lib.aqg_gen_column(self.ctx, col, C.c_uint64(seed), C.c_uint64(row_base), C.c_uint32(n),
                                          C.c_uint64(n_total), C.c_uint32(K), C.c_void_p(out.ptr)), "aqg_gen_column")
        return out

    # -- element-wise
    def ewise(self, op, l, r, ot=None, keep=False, out=None):
        l_vec = isinstance(l, DevBuf) or np.ndim(l) > 0
        r_vec = isinstance(r, DevBuf) or np.ndim(r) > 0
        kind = VEC_VEC if (l_vec and r_vec) else (VEC_SCALAR if l_vec else SCALAR_VEC)
        ld = self._dev(l) if l_vec else None
        rd = self._dev(r) if r_vec else None
        ls = None if l_vec else np.atleast_1d(np.asarray(l))
        rs = None if r_vec else np.atleast_1d(np.asarray(r))
        lt = ld.tag if l_vec else tag_of(ls)
        rt = rd.tag if r_vec else tag_of(rs)
        n = ld.n if l_vec else rd.n
        if ot is None:
            ot = self.lib.aqg_ewise_out_dtype(op, lt, rt)
        if ot == ERROR:
            raise AqgError("aqg_ewise_out_dtype", ERROR)
        out = out if out is not None else self.empty(n, TAG2NP[ot])
        lp = C.c_void_p(ld.ptr) if l_vec else ls.ctypes.data_as(C.c_void_p)
        rp = C.c_void_p(rd.ptr) if r_vec else rs.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.aqg_ewise(self.ctx, op, kind, lt, lp, rt, rp, ot, C.c_void_p(out.ptr), C.c_uint32(n)), "aqg_ewise")
        return out if keep else out.to_host()

    def unary(self, op, x, param=0):
        xd = self._dev(x)
        ot = DOUBLE if op == 0 else xd.tag
        out = self.empty(xd.n, TAG2NP[ot])
        self._chk(self.lib.aqg_unary(self.ctx, op, xd.tag, C.c_void_p(xd.ptr), C.c_uint32(xd.n), C.c_uint32(param), ot,
                                     C.c_void_p(out.ptr)), "aqg_unary")
        return out.to_host()

    # -- reductions
    def reduce(self, op, x):
        xd = self._dev(x)
        buf = (C.c_ubyte * 16)()
        self._chk(self.lib.aqg_reduce(self.ctx, op, xd.tag, C.c_void_p(xd.ptr), C.c_uint32(xd.n), buf), "aqg_reduce")
        ot = self.lib.aqg_reduce_out_dtype(op, xd.tag)
        v = np.frombuffer(bytes(buf), dtype=TAG2NP[ot], count=1)[0]
        if ot in (INT128, UINT128):
            lo, hi = int(v["lo"]), int(v["hi"])
            return (hi << 64) + lo if ot == INT128 else (hi << 64) | lo
        return v

    def corr(self, x, y):
        xd, yd = self._dev(x), self._dev(y)
        out = C.c_double()
        self._chk(self.lib.aqg_corr(self.ctx, xd.tag, C.c_void_p(xd.ptr), yd.tag, C.c_void_p(yd.ptr), C.c_uint32(xd.n),
                                    C.byref(out)), "aqg_corr")
        return out.value

    # -- scans
    def scan(self, op, x, w=0, keep=False, out=None):
        xd = self._dev(x)
        ot = self.lib.aqg_scan_out_dtype(op, xd.tag)
        out = out if out is not None else self.empty(xd.n, TAG2NP[ot])
        self._chk(self.lib.aqg_scan(self.ctx, op, xd.tag, C.c_void_p(xd.ptr), C.c_uint32(xd.n), C.c_uint32(w),
                                    C.c_void_p(out.ptr)), "aqg_scan")
        return out if keep else out.to_host()

    def scan_resume(self, op, x, carry, row_offset, keep=False, out=None):
        """sums / avgs of one row-range shard: `carry` = sum of every earlier row (python int for integer columns, float for
        floating ones), `row_offset` = number of earlier rows (aqg_scan_resume)"""
        xd = self._dev(x)
        ot = self.lib.aqg_scan_out_dtype(op, xd.tag)
        out = out if out is not None else self.empty(xd.n, TAG2NP[ot])
        if np.issubdtype(xd.dtype, np.floating):
            raw = np.array([float(carry), 0.0], dtype=np.float64).tobytes()
        else:
            raw = (int(carry) & ((1 << 128) - 1)).to_bytes(16, "little")
        buf = C.create_string_buffer(raw, 16)
        self._chk(self.lib.aqg_scan_resume(self.ctx, op, xd.tag, C.c_void_p(xd.ptr), C.c_uint32(xd.n), buf, C.c_uint64(int(row_offset)),
                                           C.c_void_p(out.ptr)), "aqg_scan_resume")
        return out if keep else out.to_host()

    # -- gather / filter
    def gather(self, x, idx):
        xd, idd = self._dev(x), self._dev(np.ascontiguousarray(idx, dtype=np.uint32) if not isinstance(idx, DevBuf) else idx)
        out = self.empty(idd.n, xd.dtype)
        self._chk(self.lib.aqg_gather(self.ctx, xd.tag, C.c_void_p(xd.ptr), C.c_void_p(idd.ptr), C.c_uint32(idd.n),
                                      C.c_void_p(out.ptr)), "aqg_gather")
        return out.to_host()

    def compact(self, x, mask):
        xd = self._dev(x)
        md = self._dev(np.ascontiguousarray(mask).astype(np.uint8) if not isinstance(mask, DevBuf) else mask)
        out = self.empty(xd.n, xd.dtype)
        m = C.c_uint32()
        self._chk(self.lib.aqg_compact(self.ctx, xd.tag, C.c_void_p(xd.ptr), C.c_void_p(md.ptr), C.c_uint32(xd.n),
                                       C.c_void_p(out.ptr), C.byref(m)), "aqg_compact")
        return out.to_host()[:m.value].copy()

    def mask_to_index(self, mask):
        md = self._dev(np.ascontiguousarray(mask).astype(np.uint8) if not isinstance(mask, DevBuf) else mask)
        out = self.empty(md.n, np.uint32)
        m = C.c_uint32()
        self._chk(self.lib.aqg_mask_to_index(self.ctx, C.c_void_p(md.ptr), C.c_uint32(md.n), C.c_void_p(out.ptr), C.byref(m)),
                  "aqg_mask_to_index")
        return out.to_host()[:m.value].copy()

    # -- sort
    def sort_rows(self, keys, orders, rows=None, out=None, keep=False):
        """aqg_sort_rows: np.uint32 row ids ordered by `keys` (key 0 most significant; numpy arrays or DevBufs of one length n)
        under `orders` (ORDER_ASC / ORDER_DESC / ORDER_NEG per key), stable.  `rows`: the row ids to order (repeats allowed),
        default every row.  `out`: a DevBuf to write into (it may be `rows` itself); keep=True returns the DevBuf."""
        kd, dts, ptrs = self._keyargs(keys)
        n = kd[0].n if kd else 0
        rd = None if rows is None else self._dev(np.ascontiguousarray(rows, dtype=np.uint32) if not isinstance(rows, DevBuf) else rows)
        m = n if rd is None else rd.n
        if out is None:
            out = self.empty(m, np.uint32)
        oa = (C.c_int * max(1, len(orders)))(*orders)
        self._chk(self.lib.aqg_sort_rows(self.ctx, len(kd), dts, ptrs, oa, C.c_uint32(n), C.c_void_p(rd.ptr) if rd is not None else None,
                                         C.c_uint32(m), C.c_void_p(out.ptr)), "aqg_sort_rows")
        return out if keep else out.to_host()

    def sort_last_passes(self):
        """digit passes the last sort_rows on this device ran (skipped digit positions not counted)"""
        p = C.c_uint32()
        self._chk(self.lib.aqg_sort_last_passes(self.ctx, C.byref(p)), "aqg_sort_last_passes")
        return p.value

    # -- median (a radix selection: include/aqg.h, median section)
    def median(self, x, which=SEL_LOWER):
        """the lower / upper median of a column, in the column's own dtype (0 for an empty column)"""
        xd = self._dev(x)
        buf = (C.c_ubyte * 16)()
        self._chk(self.lib.aqg_median(self.ctx, which, xd.tag, xd.ptr, xd.n, buf), "aqg_median")
        return np.frombuffer(bytes(buf), dtype=TAG2NP[xd.tag], count=1)[0]

    def grouped_median(self, gb, x, which=SEL_LOWER, flat=False, keep=False, out=None):
        """the median of every group of a build: `x` in row layout, or (flat=True) already in the flat layout"""
        xd = self._dev(x)
        out = out if out is not None else self.empty(gb.ngroups, TAG2NP[xd.tag])
        fn = self.lib.aqg_grouped_median_flat if flat else self.lib.aqg_grouped_median
        self._chk(fn(self.ctx, gb.h, which, xd.tag, xd.ptr, out.ptr), "aqg_grouped_median")
        return out if keep else out.to_host()

    def select_last_routes(self):
        """(mask of ROUTE_* the groups of the last median call took, most digit passes any group needed)"""
        r, p = C.c_uint32(), C.c_uint32()
        self._chk(self.lib.aqg_select_last_routes(self.ctx, C.byref(r), C.byref(p)), "aqg_select_last_routes")
        return r.value, p.value

    # -- top-k (a selection built on the median's: include/aqg.h, top-k section)
    def topk(self, x, k, order=ORDER_DESC, rows=False):
        """the k largest (ORDER_DESC) or smallest (ORDER_ASC) elements of a column, in that order: k elements of the column's dtype,
        zero past min(k, n); rows=True: also their row indices (np.uint32, 0xFFFFFFFF past min(k, n))"""
        xd = self._dev(x)
        vals = self.empty(max(int(k), 0), TAG2NP[xd.tag])
        rid = self.empty(max(int(k), 0), np.uint32) if rows else None
        self._chk(self.lib.aqg_topk(self.ctx, order, xd.tag, xd.ptr, xd.n, k, vals.ptr, rid.ptr if rows else None), "aqg_topk")
        return (vals.to_host(), rid.to_host()) if rows else vals.to_host()

    def grouped_topk(self, gb, x, k, order=ORDER_DESC, flat=False, pos=False):
        """the top k of every group of a build, a (G, k) array: `x` in row layout, or (flat=True) already in the flat layout.
        pos=True: also the (G, k) np.uint32 flat-layout positions of the elements (0xFFFFFFFF past a group's rows)"""
        xd = self._dev(x)
        G = gb.ngroups
        vals = self.empty(G * max(int(k), 0), TAG2NP[xd.tag])
        pd = self.empty(G * max(int(k), 0), np.uint32) if pos else None
        fn = self.lib.aqg_grouped_topk_flat if flat else self.lib.aqg_grouped_topk
        self._chk(fn(self.ctx, gb.h, order, xd.tag, xd.ptr, k, vals.ptr, pd.ptr if pos else None), "aqg_grouped_topk")
        v = vals.to_host().reshape(G, int(k))
        return (v, pd.to_host().reshape(G, int(k))) if pos else v

    # -- quantiles (several ranks in one selection: include/aqg.h, quantiles section)
    def quantiles(self, x, nums, den, which=SEL_LOWER):
        """the rows of rank floor (SEL_LOWER) / ceil (SEL_UPPER) of nums[j] * (n - 1) / den of a column in ascending order, len(nums)
        elements of the column's own dtype in the order of `nums` (zeros for an empty column)"""
        xd = self._dev(x)
        nq = len(nums)
        na = (C.c_uint32 * max(1, nq))(*nums)
        out = np.zeros(max(1, nq), TAG2NP[xd.tag])
        self._chk(self.lib.aqg_quantiles(self.ctx, which, nq, na, den, xd.tag, xd.ptr, xd.n, out.ctypes.data), "aqg_quantiles")
        return out[:nq]

    def grouped_quantiles(self, gb, x, nums, den, which=SEL_LOWER, flat=False, keep=False, out=None):
        """the quantiles nums[j] / den of every group of a build, a (G, len(nums)) array: `x` in row layout, or (flat=True) already
        in the flat layout"""
        xd = self._dev(x)
        nq, G = len(nums), gb.ngroups
        na = (C.c_uint32 * max(1, nq))(*nums)
        out = out if out is not None else self.empty(G * nq, TAG2NP[xd.tag])
        fn = self.lib.aqg_grouped_quantiles_flat if flat else self.lib.aqg_grouped_quantiles
        self._chk(fn(self.ctx, gb.h, which, nq, na, den, xd.tag, xd.ptr, out.ptr), "aqg_grouped_quantiles")
        return out if keep else out.to_host().reshape(G, nq)

    # -- moving quantiles (rank tracking over every row's window: include/aqg.h, moving quantiles section)
    def window_quantiles(self, x, nums, den, w, which=SEL_LOWER, keep=False, out=None):
        """the rows of rank floor (SEL_LOWER) / ceil (SEL_UPPER) of nums[j] * (len - 1) / den of every row's window (the last
        min(w, i + 1) rows) in ascending order: a (len(nums), n) array of the column's own dtype; nums = [1], den = 2 is medianw"""
        xd = self._dev(x)
        nq = len(nums)
        na = (C.c_uint32 * max(1, nq))(*nums)
        out = out if out is not None else self.empty(nq * xd.n, TAG2NP[xd.tag])
        self._chk(self.lib.aqg_window_quantiles(self.ctx, which, nq, na, den, xd.tag, xd.ptr, xd.n, w, out.ptr), "aqg_window_quantiles")
        return out if keep else out.to_host().reshape(nq, xd.n)

    def grouped_window_quantiles(self, gb, x, nums, den, w, which=SEL_LOWER, flat=False, keep=False, out=None):
        """window_quantiles within every group of a build, a (len(nums), n) array in the flat layout: `x` in row layout, or
        (flat=True) already in the flat layout"""
        xd = self._dev(x)
        nq = len(nums)
        na = (C.c_uint32 * max(1, nq))(*nums)
        out = out if out is not None else self.empty(nq * xd.n, TAG2NP[xd.tag])
        fn = self.lib.aqg_grouped_window_quantiles_flat if flat else self.lib.aqg_grouped_window_quantiles
        self._chk(fn(self.ctx, gb.h, which, nq, na, den, xd.tag, xd.ptr, w, out.ptr), "aqg_grouped_window_quantiles")
        return out if keep else out.to_host().reshape(nq, xd.n)

    def window_quantiles_last(self):
        """(rows a workgroup owns, halo rows in front of them) of the last window_quantiles / grouped_window_quantiles call"""
        t, h = C.c_uint32(), C.c_uint32()
        self._chk(self.lib.aqg_window_quantiles_last(self.ctx, C.byref(t), C.byref(h)), "aqg_window_quantiles_last")
        return t.value, h.value

    # -- ranking (comparison counting in LDS / stable sort + one rank-emit pass: include/aqg.h, ranking section)
    def rank_out(self, method, n):
        """the device column a rank call of `method` over n rows writes: uint32, or float64 for RANK_AVERAGE / PERCENT / CUME_DIST"""
        tag = self.lib.aqg_rank_out_dtype(method)
        return self.empty(n, TAG2NP[tag] if tag >= 0 else np.uint32)

    def rank(self, x, method, order=ORDER_ASC, k=0, keep=False, out=None):
        """where every row stands in the whole column, 1-based: RANK_MIN / MAX / DENSE / FIRST / NTILE (k buckets) as uint32,
        RANK_AVERAGE / PERCENT / CUME_DIST as float64; ties and NaNs as aqg_sort_rows orders them"""
        xd = self._dev(x)
        out = out if out is not None else self.rank_out(method, xd.n)
        self._chk(self.lib.aqg_rank(self.ctx, method, order, k, xd.tag, xd.ptr, xd.n, out.ptr), "aqg_rank")
        return out if keep else out.to_host()

    def grouped_rank(self, gb, x, method, order=ORDER_ASC, k=0, flat=False, keep=False, out=None):
        """rank within every group of a build, n values in the flat layout: `x` in row layout, or (flat=True) already in the flat layout"""
        xd = self._dev(x)
        out = out if out is not None else self.rank_out(method, xd.n)
        fn = self.lib.aqg_grouped_rank_flat if flat else self.lib.aqg_grouped_rank
        self._chk(fn(self.ctx, gb.h, method, order, k, xd.tag, xd.ptr, out.ptr), "aqg_grouped_rank")
        return out if keep else out.to_host()

    def rank_last(self):
        """(mask of RANK_ROUTE_* the last rank call took, sorted entries one workgroup of its emit kernel owns)"""
        r, t = C.c_uint32(), C.c_uint32()
        self._chk(self.lib.aqg_rank_last(self.ctx, C.byref(r), C.byref(t)), "aqg_rank_last")
        return r.value, t.value

    # -- pair windows (moving and running cov / corr / beta of two columns: include/aqg_pair.h)
    def scan2(self, op, x, y, w=0, keep=False, out=None):
        """SCAN2_COVW / CORRW / BETAW over the last min(w, i + 1) rows of the two columns, or the running SCAN2_COVS / CORRS / BETAS (w
        ignored): n doubles, population moments, beta = the slope of y on x"""
        xd, yd = self._dev(x), self._dev(y)
        assert xd.n == yd.n
        out = out if out is not None else self.empty(xd.n, np.float64)
        self._chk(self.lib.aqg_scan2(self.ctx, op, xd.tag, xd.ptr, yd.tag, yd.ptr, xd.n, w, out.ptr), "aqg_scan2")
        return out if keep else out.to_host()

    def grouped_scan2(self, gb, op, x, y, w=0, flat=False, keep=False, out=None):
        """the same within every group of a build, n doubles in the flat layout: `x`, `y` in row layout, or (flat=True) already flat"""
        xd, yd = self._dev(x), self._dev(y)
        assert xd.n == yd.n
        out = out if out is not None else self.empty(xd.n, np.float64)
        fn = self.lib.aqg_grouped_scan2_flat if flat else self.lib.aqg_grouped_scan2
        self._chk(fn(self.ctx, gb.h, op, xd.tag, xd.ptr, yd.tag, yd.ptr, w, out.ptr), "aqg_grouped_scan2")
        return out if keep else out.to_host()

    def scan2_last(self):
        """(SCAN2_ROUTE_* of the last scan2 / grouped_scan2 call, rows one workgroup of it owns)"""
        r, t = C.c_uint32(), C.c_uint32()
        self._chk(self.lib.aqg_scan2_last(self.ctx, C.byref(r), C.byref(t)), "aqg_scan2_last")
        return r.value, t.value

    # -- exponential moving averages (ordered scan of affine maps: include/aqg.h, exponential moving averages section)
    def ema(self, x, alpha=None, decay=None, mode=EMA_RECURSIVE, keep=False, out=None):
        """y[i] = b_i x[i] + a_i y[i-1] (EMA_RECURSIVE) or its bias-corrected form N[i] / D[i] (EMA_ADJUSTED) over the whole column:
        a constant `alpha` (a_i = 1 - alpha), or a `decay` column of doubles (a_i = decay[i]); n doubles"""
        xd = self._dev(x)
        dd = self._dev(np.asarray(decay, np.float64) if not isinstance(decay, DevBuf) else decay) if decay is not None else None
        out = out if out is not None else self.empty(xd.n, np.float64)
        self._chk(self.lib.aqg_scan_ema(self.ctx, mode, xd.tag, xd.ptr, xd.n, 0.0 if alpha is None else float(alpha), dd.ptr if dd else None, out.ptr), "aqg_scan_ema")
        return out if keep else out.to_host()

    def grouped_ema(self, gb, x, alpha=None, decay=None, mode=EMA_RECURSIVE, flat=False, keep=False, out=None):
        """ema within every group of a build, n doubles in the flat layout: `x` (and `decay`) in row layout, or (flat=True) already
        in the flat layout"""
        xd = self._dev(x)
        dd = self._dev(np.asarray(decay, np.float64) if not isinstance(decay, DevBuf) else decay) if decay is not None else None
        out = out if out is not None else self.empty(xd.n, np.float64)
        fn = self.lib.aqg_grouped_ema_flat if flat else self.lib.aqg_grouped_ema
        self._chk(fn(self.ctx, gb.h, mode, xd.tag, xd.ptr, 0.0 if alpha is None else float(alpha), dd.ptr if dd else None, out.ptr), "aqg_grouped_ema")
        return out if keep else out.to_host()

    def decay_from_times(self, t, halflife, gb=None, keep=False, out=None):
        """decay[i] = 2^(-|t[i] - t[i-1]| / halflife), decay[0] = 1: the decay column of a time-decayed ema (numeric times, or a
        key_col of DATE / TIME); gb: `t` is in the flat layout of that build, and every group's first decay is 1"""
        td = self._dev(t)
        out = out if out is not None else self.empty(td.n, np.float64)
        if gb is not None:
            self._chk(self.lib.aqg_grouped_decay_from_times_flat(self.ctx, gb.h, td.tag, td.ptr, float(halflife), out.ptr), "aqg_grouped_decay_from_times_flat")
        else:
            self._chk(self.lib.aqg_decay_from_times(self.ctx, td.tag, td.ptr, td.n, float(halflife), out.ptr), "aqg_decay_from_times")
        return out if keep else out.to_host()

    # -- time-range windows (binary-searched bounds + a combining-only block tree: include/aqg.h, time-range windows section)
    def rangew_out(self, op, x, n):
        """an empty device column for the result of `op` over the column x (None for RANGEW_COUNT)"""
        tag = self.lib.aqg_rangew_out_dtype(op, x.tag if x is not None else INT32)
        if tag == ERROR:
            raise AqgError("aqg_rangew_out_dtype", 2)
        return self.empty(n, TAG2NP[tag])

    def rangew_bounds(self, t, span, frame=RANGEW_OPEN, gb=None, keep=False, out=None):
        """lo[i] = the first position of row i's window (rows within `span` of t[i], ending at i); gb: `t` is in the flat layout of
        that build and every window is clamped at its group's start"""
        td = self._dev(t)
        out = out if out is not None else self.empty(td.n, np.uint32)
        if gb is not None:
            self._chk(self.lib.aqg_grouped_rangew_bounds_flat(self.ctx, gb.h, td.tag, td.ptr, float(span), frame, out.ptr), "aqg_grouped_rangew_bounds_flat")
        else:
            self._chk(self.lib.aqg_rangew_bounds(self.ctx, td.tag, td.ptr, td.n, float(span), frame, out.ptr), "aqg_rangew_bounds")
        return out if keep else out.to_host()

    def rangew_fold(self, op, x, lo, keep=False, out=None):
        """out[i] = op over x[lo[i] .. i] (lo[i] > i is clamped to i); x may be None for RANGEW_COUNT"""
        xd = self._dev(x) if x is not None else None
        ld = self._dev(np.asarray(lo, np.uint32) if not isinstance(lo, DevBuf) else lo)
        out = out if out is not None else self.rangew_out(op, xd, ld.n)
        self._chk(self.lib.aqg_rangew_fold(self.ctx, op, xd.tag if xd else INT32, xd.ptr if xd else None, ld.n, ld.ptr, out.ptr), "aqg_rangew_fold")
        return out if keep else out.to_host()

    def rangew(self, op, t, span, x=None, frame=RANGEW_OPEN, keep=False, out=None):
        """op over every row's time window of a column: the rows within `span` of t[i], ending at row i"""
        td = self._dev(t)
        xd = self._dev(x) if x is not None else None
        out = out if out is not None else self.rangew_out(op, xd, td.n)
        self._chk(self.lib.aqg_rangew(self.ctx, op, td.tag, td.ptr, float(span), frame, xd.tag if xd else INT32, xd.ptr if xd else None, td.n, out.ptr), "aqg_rangew")
        return out if keep else out.to_host()

    def grouped_rangew(self, gb, op, t, span, x=None, frame=RANGEW_OPEN, flat=False, keep=False, out=None):
        """rangew within every group of a build, in the flat layout: `t` and `x` in row layout, or (flat=True) already in the flat layout"""
        td = self._dev(t)
        xd = self._dev(x) if x is not None else None
        out = out if out is not None else self.rangew_out(op, xd, td.n)
        fn = self.lib.aqg_grouped_rangew_flat if flat else self.lib.aqg_grouped_rangew
        self._chk(fn(self.ctx, gb.h, op, td.tag, td.ptr, float(span), frame, xd.tag if xd else INT32, xd.ptr if xd else None, out.ptr), "aqg_grouped_rangew")
        return out if keep else out.to_host()

    def rangew_last(self):
        """(levels, rows per block at each level, rising steps, falling steps): the geometry of the last fold and the step counters
        of the last bounds pass; synchronises the stream"""
        nl, up, down = C.c_uint32(), C.c_uint32(), C.c_uint32()
        br = (C.c_uint32 * 8)()
        self._chk(self.lib.aqg_rangew_last(self.ctx, C.byref(nl), br, C.byref(up), C.byref(down)), "aqg_rangew_last")
        return nl.value, list(br)[:nl.value], up.value, down.value

    # -- count distinct (include/aqg.h, count distinct section)
    def count_distinct(self, x):
        """count(distinct x) of a column: -0.0 == +0.0, every NaN row a value of its own (0 for an empty column)"""
        xd = self._dev(x)
        out = C.c_uint32()
        self._chk(self.lib.aqg_count_distinct(self.ctx, xd.tag, xd.ptr, xd.n, C.byref(out)), "aqg_count_distinct")
        return out.value

    def grouped_count_distinct(self, gb, x, layout="row", keep=False, out=None):
        """count(distinct x) of every group of a build (np.uint32): `x` in row layout, or (layout="flat") already in the flat layout"""
        assert layout in ("row", "flat")
        xd = self._dev(x)
        out = out if out is not None else self.empty(gb.ngroups, np.uint32)
        fn = self.lib.aqg_grouped_count_distinct_flat if layout == "flat" else self.lib.aqg_grouped_count_distinct
        self._chk(fn(self.ctx, gb.h, xd.tag, xd.ptr, out.ptr), "aqg_grouped_count_distinct")
        return out if keep else out.to_host()

    def distinct_last(self):
        """(rows per tile, groups of the last count-distinct call that crossed a tile edge, (group, value) pairs they left)"""
        t, c, p = C.c_uint32(), C.c_uint32(), C.c_uint64()
        self._chk(self.lib.aqg_distinct_last(self.ctx, C.byref(t), C.byref(c), C.byref(p)), "aqg_distinct_last")
        return t.value, c.value, p.value

    # -- group by
    def _keyargs(self, keys):
        kd = [self._dev(k) for k in keys]
        dts = (C.c_int * len(kd))(*[k.tag for k in kd])
        ptrs = (C.c_void_p * len(kd))(*[k.ptr for k in kd])
        return kd, dts, ptrs

    def groupby_build(self, keys, hint=0):
        kd, dts, ptrs = self._keyargs(keys)
        h = C.c_void_p()
        self._chk(self.lib.aqg_groupby_build(self.ctx, len(kd), dts, ptrs, C.c_uint32(kd[0].n), C.c_uint32(hint), C.byref(h)),
                  "aqg_groupby_build")
        gb = GroupBy(self, h)
        gb._keep = kd
        return gb

    def groupby_agg(self, keys, ops, vals, hint=0, handle=None):
        kd, dts, ptrs = self._keyargs(keys)
        vd = [self._dev(v) if v is not None else None for v in vals]
        vdt = (C.c_int * len(vd))(*[(v.tag if v is not None else INT32) for v in vd])
        vp = (C.c_void_p * len(vd))(*[(v.ptr if v is not None else None) for v in vd])
        opa = (C.c_int * len(ops))(*ops)
        h = handle.h if handle is not None else C.c_void_p()
        self._chk(self.lib.aqg_groupby_agg(self.ctx, len(kd), dts, ptrs, len(ops), opa, vdt, vp, C.c_uint32(kd[0].n),
                                           C.c_uint32(hint), C.byref(h)), "aqg_groupby_agg")
        gb = handle if handle is not None else GroupBy(self, h)
        gb._keep = (kd, vd)            # keys of non-integer columns are fetched from the caller's column: keep the uploads alive
        gb._val_tags = [v.tag if v is not None else INT32 for v in vd]
        gb._ops = list(ops)
        return gb

    def prepare_groupby_agg(self, keys, ops, vals, hint=0):
        """the same call as groupby_agg with its argument arrays marshalled once: returns a function that runs it again on the
        same device columns and handle (a prepared statement; the per-call Python work drops to one foreign call)"""
        kd, dts, ptrs = self._keyargs(keys)
        vd = [self._dev(v) if v is not None else None for v in vals]
        vdt = (C.c_int * len(vd))(*[(v.tag if v is not None else INT32) for v in vd])
        vp = (C.c_void_p * len(vd))(*[(v.ptr if v is not None else None) for v in vd])
        opa = (C.c_int * len(ops))(*ops)
        h = C.c_void_p()
        args = (self.ctx, len(kd), dts, ptrs, len(ops), opa, vdt, vp, C.c_uint32(kd[0].n), C.c_uint32(hint), C.byref(h))
        fn, chk = self.lib.aqg_groupby_agg, self._chk
        gb = GroupBy(self, h)                      # the handle is created by the first run
        gb._val_tags = [v.tag if v is not None else INT32 for v in vd]
        gb._ops = list(ops)
        gb._keep = (kd, vd, dts, ptrs, vdt, vp, opa)

        def run():
            rc = fn(*args)
            if rc != 0:
                chk(rc, "aqg_groupby_agg")
            return gb
        return run, gb

    def join_groupby_sum(self, dim_keys, dim_vals, fact_fk, group_keys, fact_vals, hint=0, handle=None):
        """fact JOIN dim ON fk = key, then sum(val * w) by group key -- one fused pass (aqg_join_groupby_sum)"""
        dk, dv, fk, gk, fv = (self._dev(a) for a in (dim_keys, dim_vals, fact_fk, group_keys, fact_vals))
        h = handle.h if handle is not None else C.c_void_p()
        self._chk(self.lib.aqg_join_groupby_sum(self.ctx, dk.tag, C.c_void_p(dk.ptr), dv.tag, C.c_void_p(dv.ptr), C.c_uint32(dk.n),
                                                C.c_void_p(fk.ptr), gk.tag, C.c_void_p(gk.ptr), fv.tag, C.c_void_p(fv.ptr), C.c_uint32(fk.n),
                                                C.c_uint32(hint), C.byref(h)), "aqg_join_groupby_sum")
        gb = handle if handle is not None else GroupBy(self, h)
        gb._keep = (dk, dv, fk, gk, fv)
        return gb
    def groupby_pack(self, gb, agg_index, gmax, out_ptr):
        """exchange payload of a shard's group table: (gmax + 1) int64 pairs at device address `out_ptr` (aqg_groupby_pack)"""
        self._chk(self.lib.aqg_groupby_pack(gb.h, agg_index, C.c_uint32(gmax), C.c_void_p(out_ptr)), "aqg_groupby_pack")
    def groupby_merge_packed(self, gathered_ptr, world, gmax, key_tag, op, handle=None):
        """merge the gathered payloads of `world` shards (aqg_groupby_merge_packed)"""
        h = handle.h if handle is not None else C.c_void_p()
        self._chk(self.lib.aqg_groupby_merge_packed(self.ctx, C.c_void_p(gathered_ptr), C.c_uint32(world), C.c_uint32(gmax), key_tag, op, C.byref(h)),
                  "aqg_groupby_merge_packed")
        return handle if handle is not None else GroupBy(self, h)
    def grouped_reduce(self, gb, op, x):
        xd = self._dev(x)
        ot = self.lib.aqg_reduce_out_dtype(op, xd.tag)
        out = self.empty(gb.ngroups, TAG2NP[ot])
        self._chk(self.lib.aqg_grouped_reduce(self.ctx, gb.h, op, xd.tag, C.c_void_p(xd.ptr), C.c_void_p(out.ptr)), "aqg_grouped_reduce")
        self.sync()
        return out.to_host()

    # -- per-group scans / windows / two-column aggregates over the flat layout of a build (include/aqg.h)
    def group_offsets(self, gb):
        self.lib.aqg_groupby_offsets.restype = C.c_void_p
        p = self.lib.aqg_groupby_offsets(gb.h)
        assert p, "aqg_groupby_offsets"
        return DevBuf(self, p, np.uint32, gb.ngroups + 1, owned=False).to_host()

    def grouped_flatten(self, gb, x, keep=False):
        xd = self._dev(x)
        out = self.empty(xd.n, xd.dtype)
        self._chk(self.lib.aqg_grouped_flatten(self.ctx, gb.h, xd.tag, C.c_void_p(xd.ptr), C.c_void_p(out.ptr)), "aqg_grouped_flatten")
        return out if keep else out.to_host()

    def grouped_scan(self, gb, op, x, w=0, flat=False, keep=False, out=None):
        """per-group scan of a column: `x` in row layout (flat=False: flatten + scan in one call) or already flat"""
        xd = self._dev(x)
        ot = self.lib.aqg_scan_out_dtype(op, xd.tag)
        out = out if out is not None else self.empty(xd.n, TAG2NP[ot])
        fn = self.lib.aqg_grouped_scan_flat if flat else self.lib.aqg_grouped_scan
        self._chk(fn(self.ctx, gb.h, op, xd.tag, C.c_void_p(xd.ptr), C.c_uint32(w), C.c_void_p(out.ptr)), "aqg_grouped_scan")
        return out if keep else out.to_host()

    def grouped_reduce_flat(self, gb, op, xflat):
        xd = self._dev(xflat)
        ot = self.lib.aqg_reduce_out_dtype(op, xd.tag)
        out = self.empty(gb.ngroups, TAG2NP[ot])
        self._chk(self.lib.aqg_grouped_reduce_flat(self.ctx, gb.h, op, xd.tag, C.c_void_p(xd.ptr), C.c_void_p(out.ptr)), "aqg_grouped_reduce_flat")
        self.sync()
        return out.to_host()

    def grouped_corr(self, gb, x, y):
        xd, yd = self._dev(x), self._dev(y)
        out = self.empty(gb.ngroups, np.float64)
        self._chk(self.lib.aqg_grouped_corr(self.ctx, gb.h, xd.tag, C.c_void_p(xd.ptr), yd.tag, C.c_void_p(yd.ptr), C.c_void_p(out.ptr)), "aqg_grouped_corr")
        self.sync()
        return out.to_host()

    def grouped_ewise(self, gb, op, v, s, kind=VEC_SCALAR, layout=LAYOUT_ROW, ot=None, keep=False, out=None):
        """out[i] = v[i] OP s[group of i] (kind=VEC_SCALAR) or s[group of i] OP v[i] (kind=SCALAR_VEC) for all groups of a build in
        one launch: `v` in row layout, or (layout=LAYOUT_FLAT) in the flat layout; `s`: one scalar per group"""
        vd, sd = self._dev(v), self._dev(s)
        if ot is None:
            ot = self.lib.aqg_ewise_out_dtype(op, *((vd.tag, sd.tag) if kind == VEC_SCALAR else (sd.tag, vd.tag)))
        if ot == ERROR:
            raise AqgError("aqg_ewise_out_dtype", ERROR)
        out = out if out is not None else self.empty(vd.n, TAG2NP[ot])
        self._chk(self.lib.aqg_grouped_ewise(self.ctx, gb.h, layout, op, kind, vd.tag, C.c_void_p(vd.ptr), sd.tag, C.c_void_p(sd.ptr), ot,
                                             C.c_void_p(out.ptr)), "aqg_grouped_ewise")
        return out if keep else out.to_host()

    # -- join
    def join_pairs(self, build, probe):
        bd, pd = self._dev(build), self._dev(probe)
        m = C.c_uint64()
        self._chk(self.lib.aqg_join_count(self.ctx, bd.tag, C.c_void_p(bd.ptr), C.c_uint32(bd.n), C.c_void_p(pd.ptr),
                                          C.c_uint32(pd.n), C.byref(m)), "aqg_join_count")
        pr, br = self.empty(m.value, np.uint32), self.empty(m.value, np.uint32)
        self._chk(self.lib.aqg_join_pairs(self.ctx, bd.tag, C.c_void_p(bd.ptr), C.c_uint32(bd.n), C.c_void_p(pd.ptr),
                                          C.c_uint32(pd.n), C.c_void_p(pr.ptr), C.c_void_p(br.ptr), C.c_uint64(m.value),
                                          C.byref(m)), "aqg_join_pairs")
        return pr.to_host(), br.to_host()

    def join_count(self, build, probe):
        """number of matching (probe row, build row) pairs, in 64 bits (aqg_join_count)"""
        bd, pd = self._dev(build), self._dev(probe)
        m = C.c_uint64()
        self._chk(self.lib.aqg_join_count(self.ctx, bd.tag, C.c_void_p(bd.ptr), C.c_uint32(bd.n), C.c_void_p(pd.ptr),
                                          C.c_uint32(pd.n), C.byref(m)), "aqg_join_count")
        return m.value

    def join_lookup(self, build, probe):
        bd, pd = self._dev(build), self._dev(probe)
        out = self.empty(pd.n, np.uint32)
        self._chk(self.lib.aqg_join_lookup(self.ctx, bd.tag, C.c_void_p(bd.ptr), C.c_uint32(bd.n), C.c_void_p(pd.ptr),
                                           C.c_uint32(pd.n), C.c_void_p(out.ptr)), "aqg_join_lookup")
        return out.to_host()

    # -- joins on composite and typed keys (include/aqg.h): a side is a list of key columns (numpy arrays, DevBufs, key_col results)
    def join_keys_count(self, build_cols, probe_cols, kind=JOIN_INNER):
        """the number of output rows of the join, in 64 bits (aqg_join_keys_count)"""
        bd, dts, bp = self._keyargs(build_cols)
        pd, _, pp = self._keyargs(probe_cols)
        m = C.c_uint64()
        self._chk(self.lib.aqg_join_keys_count(self.ctx, kind, len(bd), dts, bp, bd[0].n, pp, pd[0].n, C.byref(m)), "aqg_join_keys_count")
        return m.value

    def join_keys_pairs(self, build_cols, probe_cols, kind=JOIN_INNER):
        """(probe_rows, build_rows) of the join as np.uint32 arrays; build_rows is None for JOIN_SEMI / JOIN_ANTI"""
        bd, dts, bp = self._keyargs(build_cols)
        pd, _, pp = self._keyargs(probe_cols)
        m = C.c_uint64()
        self._chk(self.lib.aqg_join_keys_count(self.ctx, kind, len(bd), dts, bp, bd[0].n, pp, pd[0].n, C.byref(m)), "aqg_join_keys_count")
        pr = self.empty(m.value, np.uint32)
        br = self.empty(m.value, np.uint32) if kind in (JOIN_INNER, JOIN_LEFT) else None
        self._chk(self.lib.aqg_join_keys_pairs(self.ctx, kind, len(bd), dts, bp, bd[0].n, pp, pd[0].n, pr.ptr, br.ptr if br is not None else None,
                                               m.value, C.byref(m)), "aqg_join_keys_pairs")
        return pr.to_host()[:m.value], (br.to_host()[:m.value] if br is not None else None)

    def join_keys_lookup(self, build_cols, probe_cols):
        """np.uint32[np]: the lowest build row whose key tuple equals probe row i, else 0xFFFFFFFF"""
        bd, dts, bp = self._keyargs(build_cols)
        pd, _, pp = self._keyargs(probe_cols)
        out = self.empty(pd[0].n, np.uint32)
        self._chk(self.lib.aqg_join_keys_lookup(self.ctx, len(bd), dts, bp, bd[0].n, pp, pd[0].n, out.ptr), "aqg_join_keys_lookup")
        return out.to_host()

    def join_last(self):
        """(JOIN_ROUTE_* mask, distinct build tuples, table slots) of the last join_keys_* call on this device"""
        r, g, s = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self.lib.aqg_join_last(self.ctx, C.byref(r), C.byref(g), C.byref(s)), "aqg_join_last")
        return r.value, g.value, s.value

    def join_tuple_slots(self, cols, table_slots):
        return join_tuple_slots(cols, table_slots)

    # -- as-of join (include/aqg.h): a side is a list of 0..8 key columns, as for join_keys_*, and its `on` column
    def join_asof(self, build_cols, build_on, probe_cols, probe_on, direction=ASOF_BACKWARD, strict=False):
        """np.uint32[np]: for every probe row the build row of its key tuple with the nearest `on` at or before (ASOF_BACKWARD) or at
        or after (ASOF_FORWARD) its own -- strictly before / after under `strict` -- else 0xFFFFFFFF (aqg_join_asof)"""
        bo, po = self._dev(build_on), self._dev(probe_on)
        bd, dts, bp = self._keyargs(build_cols) if len(build_cols) else ([], None, None)
        pd, _, pp = self._keyargs(probe_cols) if len(probe_cols) else ([], None, None)
        out = self.empty(po.n, np.uint32)
        self._chk(self.lib.aqg_join_asof(self.ctx, direction, ASOF_STRICT if strict else 0, len(bd), dts, bp, bo.ptr, bo.n, pp, po.ptr, po.n, bo.tag,
                                         out.ptr), "aqg_join_asof")
        return out.to_host()

    def join_asof_last(self):
        """(ASOF_ROUTE_* mask, distinct build tuples, digit passes of the ordering step) of the last join_asof call on this device"""
        r, g, p = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self.lib.aqg_join_asof_last(self.ctx, C.byref(r), C.byref(g), C.byref(p)), "aqg_join_asof_last")
        return r.value, g.value, p.value

    # -- window join (include/aqg.h): sides as for join_asof; a window is `before` in front of and `after` behind the probe row's `on`
    def _wj_sides(self, build_cols, build_on, probe_cols, probe_on):
        bo, po = self._dev(build_on), self._dev(probe_on)
        bd, dts, bp = self._keyargs(build_cols) if len(build_cols) else ([], None, None)
        pd, _, pp = self._keyargs(probe_cols) if len(probe_cols) else ([], None, None)
        return bo, po, (bd, pd), len(bd), dts, bp, pp

    def join_window_bounds(self, build_cols, build_on, probe_cols, probe_on, before, after, flags=0, keep=False):
        """(order, lo, hi): the build rows by (group, on, row) and, per probe row, the positions [lo, hi) of that order its window
        holds (aqg_join_window_bounds); flags: WJ_OPEN_LO | WJ_OPEN_HI | WJ_PREVAILING"""
        bo, po, held, nk, dts, bp, pp = self._wj_sides(build_cols, build_on, probe_cols, probe_on)
        order, lo, hi = self.empty(bo.n, np.uint32), self.empty(po.n, np.uint32), self.empty(po.n, np.uint32)
        self._chk(self.lib.aqg_join_window_bounds(self.ctx, flags, nk, dts, bp, bo.ptr, bo.n, pp, po.ptr, po.n, bo.tag, float(before), float(after),
                                                  order.ptr, lo.ptr, hi.ptr), "aqg_join_window_bounds")
        return (order, lo, hi) if keep else (order.to_host(), lo.to_host(), hi.to_host())

    def interval_fold(self, op, x, lo, hi, fill=None, keep=False, out=None):
        """out[i] = op over x[lo[i] .. min(hi[i], n)); an empty interval gives 0 (COUNT, SUM) or `fill` (None: zero bytes); x may be
        None for RANGEW_COUNT over a column of `n` = max(hi) rows"""
        ld = self._dev(np.asarray(lo, np.uint32) if not isinstance(lo, DevBuf) else lo)
        hd = self._dev(np.asarray(hi, np.uint32) if not isinstance(hi, DevBuf) else hi)
        xd = self._dev(x) if x is not None else None
        n = xd.n if xd is not None else 0xFFF00000
        out = out if out is not None else self.rangew_out(op, xd, ld.n)
        f = None if fill is None else np.array([fill], dtype=out.dtype)
        self._chk(self.lib.aqg_interval_fold(self.ctx, op, xd.tag if xd else INT32, xd.ptr if xd else None, n, ld.ptr, hd.ptr, ld.n,
                                             f.ctypes.data if f is not None else None, out.ptr), "aqg_interval_fold")
        return out if keep else out.to_host()

    def join_window(self, op, build_cols, build_on, probe_cols, probe_on, before, after, x=None, flags=0, fill=None):
        """per probe row, `op` (RANGEW_*) over the values `x` of the build rows of its key tuple within `before` in front of and
        `after` behind its `on` (aqg_join_window); x may be None for RANGEW_COUNT"""
        bo, po, held, nk, dts, bp, pp = self._wj_sides(build_cols, build_on, probe_cols, probe_on)
        xd = self._dev(x) if x is not None else None
        out = self.rangew_out(op, xd, po.n)
        f = None if fill is None else np.array([fill], dtype=out.dtype)
        self._chk(self.lib.aqg_join_window(self.ctx, op, flags, nk, dts, bp, bo.ptr, bo.n, pp, po.ptr, po.n, bo.tag, float(before), float(after),
                                           xd.tag if xd else INT32, xd.ptr if xd else None, f.ctypes.data if f is not None else None, out.ptr),
                  "aqg_join_window")
        return out.to_host()

    def join_window_last(self):
        """(ASOF_ROUTE_* | WJ_FOLD_* mask, distinct build tuples, digit passes of the ordering step) of the last window-join call"""
        r, g, p = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self.lib.aqg_join_window_last(self.ctx, C.byref(r), C.byref(g), C.byref(p)), "aqg_join_window_last")
        return r.value, g.value, p.value

    def gather_fill(self, x, idx, fill=None):
        """out[i] = fill where idx[i] == 0xFFFFFFFF, else x[idx[i]]; fill None = zero bytes (aqg_gather_fill)"""
        xd, idd = self._dev(x), self._dev(np.ascontiguousarray(idx, dtype=np.uint32) if not isinstance(idx, DevBuf) else idx)
        out = self.empty(idd.n, xd.dtype)
        f = None if fill is None else np.array([fill], dtype=xd.dtype)
        self._chk(self.lib.aqg_gather_fill(self.ctx, xd.tag, xd.ptr, idd.ptr, idd.n, f.ctypes.data if f is not None else None, out.ptr), "aqg_gather_fill")
        return out.to_host()

    # -- timing
    def debug_ws_check(self):
        """aqg_debug_ws_check: run the scratch-memory check; the latched report as a dict (kind WS_CLEAN: nothing damaged)"""
        r = WsReport()
        self._chk(self.lib.aqg_debug_ws_check(self.ctx, C.byref(r)), "aqg_debug_ws_check")
        return {"kind": r.kind, "alloc_index": r.alloc_index, "offset": r.offset, "alloc_offset": r.alloc_offset,
                "alloc_bytes": r.alloc_bytes, "expected": r.expected, "found": r.found}

    def debug_ws_info(self):
        """aqg_debug_ws_info: the arena of the last use and its logged sub-allocations [(physical offset, bytes), ...]"""
        i = WsInfo()
        self._chk(self.lib.aqg_debug_ws_info(self.ctx, C.byref(i), None, 0), "aqg_debug_ws_info")
        a = np.zeros(2 * max(1, i.nallocs), np.uint64)
        self._chk(self.lib.aqg_debug_ws_info(self.ctx, C.byref(i), a.ctypes.data_as(C.c_void_p), i.nallocs), "aqg_debug_ws_info")
        return {"base": i.base or 0, "physical_bytes": i.physical_bytes, "logical_bytes": i.logical_bytes, "rank_bm": i.rank_bm or 0,
                "rank_bm_bytes": i.rank_bm_bytes, "guard": bool(i.guard), "pattern": i.pattern,
                "allocs": [(int(a[2 * k]), int(a[2 * k + 1])) for k in range(i.nallocs)]}

    def memset(self, ptr, byte, nbytes):
        self._chk(self.lib.aqg_memset(self.ctx, C.c_void_p(ptr), int(byte), C.c_size_t(nbytes)), "aqg_memset")

    def timer_start(self):
        self._chk(self.lib.aqg_timer_start(self.ctx), "aqg_timer_start")

    def last_kernel_ms(self):
        ms = C.c_float()
        self._chk(self.lib.aqg_last_kernel_ms(self.ctx, C.byref(ms)), "aqg_last_kernel_ms")
        return ms.value

    def timer_stop_ms(self):
        ms = C.c_float()
        self._chk(self.lib.aqg_timer_stop_ms(self.ctx, C.byref(ms)), "aqg_timer_stop_ms")
        return ms.value
