"""The as-of join (aqg_join_asof, aqg_join_asof_last) against its model (tests/asof_model.py; tests/test_asof_model.py holds that model
to its brute-force form and to recorded answers of pandas merge_asof).  Everything goes through the C-ABI; every result is a row id,
a route mask, a count or a status and is compared for equality, every row of it.  Every call writes between canary words."""
import ctypes as C
import functools

import numpy as np
import pytest

import asof_cases
import asof_model as am
import checker as ck

pytestmark = pytest.mark.gpu
NONE = am.NONE
AQG_OK, AQG_ERR_DTYPE, AQG_ERR_ARG = 0, 2, 3
STRICT = 1
CANARY = 0xA5A5A5A5
MODES = [(d, s) for d in (am.BACKWARD, am.FORWARD) for s in (False, True)]
MODE_IDS = ["backward", "backward_strict", "forward", "forward_strict"]


@pytest.fixture(scope="module")
def gpu():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


@functools.lru_cache(maxsize=None)
def want_of(name, d, s):
    bk, bo, pk, po, _ = asof_cases.cases()[name]
    return am.asof_rows_sorted(bk, bo, pk, po, d, s)


def asof_raw(gpu, bk, bo, pk, po, d, flags, shift=0, on_tag=None, nkeys=None, out_at=None, fill=CANARY):
    """aqg_join_asof with every column starting `shift` elements into its allocation and the output `4 + shift` words into one filled
    with canaries: (status, the np output words, the canaries around them are intact)"""
    keep = []

    def up(a):
        a = np.ascontiguousarray(a)
        buf = gpu.to_device(np.concatenate([np.zeros(shift, a.dtype), a]))
        keep.append(buf)
        return buf.ptr + shift * a.dtype.itemsize
    nk = len(bk)
    dts = (C.c_int * max(1, nk))(*[t for t, _ in bk])
    bp = (C.c_void_p * max(1, nk))(*[up(a) for _, a in bk])
    pp = (C.c_void_p * max(1, nk))(*[up(a) for _, a in pk])
    npr, pad = len(po), 4 + shift
    outbuf = gpu.to_device(np.full(npr + 2 * pad, fill, np.uint32))
    po_ptr = up(po)
    out_ptr = outbuf.ptr + pad * 4 if out_at is None else po_ptr
    rc = gpu.lib.aqg_join_asof(gpu.ctx, d, flags, nk if nkeys is None else nkeys, dts if nk else None, bp if nk else None, up(bo), len(bo),
                               pp if nk else None, po_ptr, npr, ck.NP2TAG[np.asarray(bo).dtype] if on_tag is None else on_tag, out_ptr)
    host = outbuf.to_host()
    return rc, host[pad:pad + npr], bool((host[:pad] == CANARY).all() and (host[pad + npr:] == CANARY).all())


def groups_of(bk, bo):
    return am.group_ids(bk, len(bo), [], 0)[1] if bk else 1


# ---- every named case, both directions, strict and not -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", sorted(asof_cases.cases()))
def test_case_equals_model(gpu, name, mode):
    bk, bo, pk, po, routes = asof_cases.cases()[name]
    d, s = mode
    rc, got, intact = asof_raw(gpu, bk, bo, pk, po, d, STRICT if s else 0)
    assert rc == AQG_OK and intact
    assert np.array_equal(got, want_of(name, d, s))
    r, G, passes = gpu.join_asof_last()
    assert r == routes and G == groups_of(bk, bo)
    if routes & am.PRESORTED:                                    # sorted by the group id alone; nothing at all without key columns
        assert passes == am.sort_passes(bk, bo)
        assert passes <= 4 and (bk or passes == 0)


@pytest.mark.parametrize("shift", [1, 3])
@pytest.mark.parametrize("name", ["np_1", "np_2", "np_3", "np_5", "lds_i64", "lds_i32", "ends_int8", "nokeys"])
def test_unaligned_device_offsets(gpu, name, shift):
    bk, bo, pk, po, routes = asof_cases.cases()[name]
    for d, s in MODES:
        rc, got, intact = asof_raw(gpu, bk, bo, pk, po, d, STRICT if s else 0, shift=shift)
        assert rc == AQG_OK and intact
        assert np.array_equal(got, want_of(name, d, s)), (d, s)
        assert gpu.join_asof_last()[0] == routes


def test_python_binding(gpu):
    from aquery2_amd import capi
    bk, bo, pk, po, routes = asof_cases.cases()["group_sizes"]
    for d, s in MODES:
        got = gpu.join_asof([a for _, a in bk], bo, [a for _, a in pk], po, direction=(capi.ASOF_BACKWARD, capi.ASOF_FORWARD)[d], strict=s)
        assert got.dtype == np.uint32 and np.array_equal(got, want_of("group_sizes", d, s))
    assert gpu.join_asof_last() == (routes, groups_of(bk, bo), am.sort_passes(bk, bo))
    bk, bo, pk, po, routes = asof_cases.cases()["nokeys_presorted"]
    assert np.array_equal(gpu.join_asof([], bo, [], po), want_of("nokeys_presorted", am.BACKWARD, False))
    assert gpu.join_asof_last() == (capi.ASOF_ROUTE_HBM | capi.ASOF_ROUTE_NOKEYS | capi.ASOF_ROUTE_PRESORTED, 1, 0)


# ---- seeded fuzz ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(40))
def test_fuzz(gpu, seed):
    bk, bo, pk, po, d, s = asof_cases.random_sides(seed, 5000)
    rc, got, intact = asof_raw(gpu, bk, bo, pk, po, d, STRICT if s else 0, shift=seed % 2)
    assert rc == AQG_OK and intact
    assert np.array_equal(got, am.asof_rows_sorted(bk, bo, pk, po, d, s))
    r, G, passes = gpu.join_asof_last()
    if len(bo):
        assert r == am.HBM | (0 if bk else am.NOKEYS) | (am.PRESORTED if am.presorted(bo) else 0) and G == groups_of(bk, bo)
    else:
        assert (r, G, passes) == (0, 0, 0)


# ---- empty sides, errors ----------------------------------------------------------------------------------------------------------------
def test_empty_sides(gpu):
    bk, bo, pk, po, _ = asof_cases.cases()["absent_keys"]
    for d, s in MODES:
        rc, got, intact = asof_raw(gpu, [(t, a[:0]) for t, a in bk], bo[:0], pk, po, d, STRICT if s else 0)
        assert rc == AQG_OK and intact and (got == NONE).all()
        assert gpu.join_asof_last() == (0, 0, 0)
        rc, got, intact = asof_raw(gpu, bk, bo, [(t, a[:0]) for t, a in pk], po[:0], d, STRICT if s else 0)
        assert rc == AQG_OK and intact and len(got) == 0
        assert gpu.join_asof_last() == (0, 0, 0)


def test_error_returns_leave_the_output_untouched(gpu):
    bk, bo, pk, po, _ = asof_cases.cases()["absent_keys"]
    i128 = np.zeros(len(bo), ck.I128)

    def refused(code, **kw):
        args = dict(bk=bk, bo=bo, pk=pk, po=po, d=am.BACKWARD, flags=0)
        args.update(kw)
        rc, got, intact = asof_raw(gpu, args.pop("bk"), args.pop("bo"), args.pop("pk"), args.pop("po"), args.pop("d"), args.pop("flags"), **args)
        assert rc == code and intact and (got == CANARY).all(), kw
        assert gpu.join_asof_last() == (0, 0, 0)
    assert asof_raw(gpu, bk, bo, pk, po, am.BACKWARD, 0)[0] == AQG_OK           # a call that leaves routes behind
    refused(AQG_ERR_ARG, d=2)
    refused(AQG_ERR_ARG, d=-1)
    refused(AQG_ERR_ARG, flags=2)
    refused(AQG_ERR_ARG, flags=3)
    for tag in (ck.BOOL, ck.INT128, ck.UINT128, ck.DATE, ck.TIME, ck.TIMESTAMP, ck.STR):
        refused(AQG_ERR_DTYPE, on_tag=tag)
    refused(AQG_ERR_DTYPE, bk=[(ck.STR, bk[0][1])], pk=[(ck.STR, pk[0][1])])
    refused(AQG_ERR_ARG, bk=[(ck.INT128, i128)] * 5, pk=[(ck.INT128, np.zeros(len(po), ck.I128))] * 5)      # ten normalised columns
    refused(AQG_ERR_ARG, nkeys=9)
    refused(AQG_ERR_ARG, nkeys=-1)
    # null columns with rows, and an output over an input
    out = gpu.to_device(np.full(len(po) + 8, CANARY, np.uint32))
    bon, pon = gpu.to_device(bo), gpu.to_device(po)
    tag = ck.NP2TAG[bo.dtype]
    call = lambda b, p, o: gpu.lib.aqg_join_asof(gpu.ctx, 0, 0, 0, None, None, b, len(bo), None, p, len(po), tag, o)
    assert call(None, pon.ptr, out.ptr + 16) == AQG_ERR_ARG
    assert call(bon.ptr, None, out.ptr + 16) == AQG_ERR_ARG
    assert call(bon.ptr, pon.ptr, None) == AQG_ERR_ARG
    assert call(bon.ptr, out.ptr + 16, out.ptr + 16) == AQG_ERR_ARG             # int16 probe column inside the output words
    assert call(out.ptr + 4 * len(po), pon.ptr, out.ptr + 16) == AQG_ERR_ARG
    assert (out.to_host() == CANARY).all()
    assert gpu.join_asof_last() == (0, 0, 0)
    assert call(bon.ptr, pon.ptr, out.ptr + 16) == AQG_OK
    assert np.array_equal(out.to_host()[4:4 + len(po)], am.asof_rows(bk[:0], bo, pk[:0], po, am.BACKWARD, False))


# ---- the outer side through aqg_gather_fill ------------------------------------------------------------------------------------------
def test_gather_fill_over_the_result(gpu):
    bk, bo, pk, po, _ = asof_cases.cases()["group_sizes"]
    rng = np.random.default_rng(5)
    price = rng.normal(100, 5, len(bo))
    for d, s in MODES:
        rows = gpu.join_asof([a for _, a in bk], bo, [a for _, a in pk], po, direction=d, strict=s)
        want = want_of("group_sizes", d, s)
        got = gpu.gather_fill(price, rows, fill=-1.0)
        assert np.array_equal(got, np.where(want == NONE, -1.0, price[np.where(want == NONE, 0, want)]))
