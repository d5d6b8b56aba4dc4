"""Decode tests/golden/ref_golden.json (made by oracle/gen_golden.py from the real reference), and answer for the reference
from tests/golden/ref_digests.json (made by oracle/gen_ref_digests.py) where it is not built."""
import hashlib
import json
import os

import numpy as np

import checker as ck

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_golden.json")
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_digests.json")
_NAME2DT = {"int128": ck.I128, "uint128": ck.U128, "bool": np.dtype(np.uint8)}


def dec(e):
    dt = _NAME2DT.get(e["dtype"], None) or np.dtype(e["dtype"])
    return np.frombuffer(bytes.fromhex(e["hex"]), dtype=dt, count=e["n"]).copy()


def dec_scalar(e):
    if "int" in e:
        return int(e["int"])
    return dec(e)[0]


def load():
    with open(PATH) as f:
        return json.load(f)["cases"]


def operand(c, side):
    a = dec(c[side])
    return a[0] if c[side + "_scalar"] else a


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype.itemsize == b.dtype.itemsize and a.tobytes() == b.tobytes()


def scalar_same(got, want):
    if isinstance(want, int) and not isinstance(want, (np.integer,)):
        return int(got) == want
    return np.asarray(got).tobytes() == np.asarray(want).tobytes()


def digest(v):
    """64-bit digest of a value's exact bits: element type, shape and bytes of an array or numpy scalar; the decimal text of a
    python int (128-bit results come back as python ints) or the repr of a float"""
    h = hashlib.sha256()
    if isinstance(v, bytes):
        h.update(b"bytes:" + v)
    elif isinstance(v, (bool, int)):
        h.update(f"{type(v).__name__}:{v}".encode())
    elif isinstance(v, float):
        h.update(b"float:" + np.float64(v).tobytes())
    else:
        a = np.ascontiguousarray(np.asarray(v))
        assert a.dtype != object, type(v)
        h.update(f"{a.dtype.str}{a.shape}:".encode() + a.tobytes())
    return h.hexdigest()[:16]


class RefAnswers:
    """The real reference's answer to each named question, compared bit for bit with what the oracle computed.  The answers are
    read from tests/golden/ref_digests.json everywhere; where oracle/_ref is built the reference is also asked live, so that a
    stale digest file fails too.  With record=True (oracle/gen_ref_digests.py) the live answers are collected and saved instead."""

    def __init__(self, live, record=False):
        assert live is not None or not record, "recording needs oracle/_ref/libaqref.so"
        self.live, self.record, self.recorded = live, record, {}
        self.stored = {}
        if os.path.exists(DIGESTS):
            with open(DIGESTS) as f:
                self.stored = json.load(f)["digests"]

    def check(self, key, got, ask):
        """`got`: the oracle's value; `ask(ref)`: the same question put to a reference library"""
        d = digest(got)
        if self.live is not None:
            want = digest(ask(self.live))
            if self.record:
                assert self.recorded.setdefault(key, want) == want, f"{key}: two different answers recorded under one name"
            assert d == want, f"{key}: the oracle differs from the live reference"
        if not self.record:
            assert key in self.stored, f"{key}: no recorded answer of the reference (oracle/gen_ref_digests.py)"
            assert d == self.stored[key], f"{key}: the oracle differs from the reference's recorded answer"

    def save(self):
        with open(DIGESTS, "w") as f:
            json.dump({"about": "sha256[:16] of the real reference's outputs (tests/golden_util.py digest), by question; "
                                "made by oracle/gen_ref_digests.py", "digests": dict(sorted(self.recorded.items()))}, f, indent=0)
            f.write("\n")
