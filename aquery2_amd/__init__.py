"""aquery2_amd -- MI355X-native execution library for the AQuery column-batch hot path.

The product is the C-ABI shared library `libaqg.so` (include/aqg.h) built from the hand-written
HIP kernels under aquery2_amd/csrc/, plus the host C++ headers under include/aquery/ that mirror
the reference's header-level API.  This Python package is a thin ctypes harness over the C-ABI
used by tests/ and bench.py; it contains no compute of its own and no CPU fallback.
"""
from . import capi  # noqa: F401
from .capi import Device, DevBuf, AqgError, Comm, ThreadRanks, lib_path, load_library  # noqa: F401
from .capi import (RANK_MIN, RANK_MAX, RANK_DENSE, RANK_FIRST, RANK_AVERAGE, RANK_PERCENT, RANK_CUME_DIST, RANK_NTILE,  # noqa: F401
                   RANK_ROUTE_SMALL, RANK_ROUTE_SORTED)
from .capi import (SCAN2_COVS, SCAN2_CORRS, SCAN2_BETAS, SCAN2_COVW, SCAN2_CORRW, SCAN2_BETAW,  # noqa: F401
                   SCAN2_ROUTE_REG, SCAN2_ROUTE_LDS, SCAN2_ROUTE_PREFIX)
