"""Runs calls of tests/scratch_catalogue.py in this process, each on a fresh Device(0), and writes one JSON line per call to a log:
the entries it called, every status, a digest of every byte that came back from the device, the `*_last` route words, the plan bits
and -- under AQG_WS_GUARD -- the guard's report.  The call's name is written and flushed BEFORE the call starts, so that a call that
takes the process down is named by the log's last line.  Stops at the first call that fails inside the HIP runtime.

    python tests/scratch_child.py LOG [--families a,b] [--switches NAME] [--names n1,n2] [--controls]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import aquery2_amd  # noqa: E402
from aquery2_amd import capi as P  # noqa: E402
import checker  # noqa: E402
import scratch_catalogue as cat  # noqa: E402

RANK = {"aqg_rank", "aqg_grouped_rank", "aqg_grouped_rank_flat"}
JOIN = {"aqg_join_keys_count", "aqg_join_keys_pairs", "aqg_join_keys_lookup"}
WJ = {"aqg_join_window_bounds", "aqg_join_window", "aqg_interval_fold"}
SELECT = {"aqg_median", "aqg_grouped_median", "aqg_grouped_median_flat", "aqg_topk", "aqg_grouped_topk", "aqg_grouped_topk_flat",
          "aqg_quantiles", "aqg_grouped_quantiles", "aqg_grouped_quantiles_flat"}


NOT_A_STATUS = {n for n, why in cat.EXEMPT.items() if why.startswith("type rule")} | {"aqg_comm_rank", "aqg_comm_world", "aqg_device_count"}
VOID = {"aqg_groupby_destroy", "aqg_ctx_destroy", "aqg_comm_destroy"}          # (no return value: whatever the register holds)


def _int(a):
    if a is None:
        return 0
    v = getattr(a, "value", a)
    return int(v or 0)


class Recorder:
    def __init__(self):
        self.h = hashlib.sha256()
        self.called = set()
        self.routes = {"rank": 0, "join": 0, "asof": 0, "wj": 0, "select": 0, "str": 0, "sort": set()}
        self.failed_in_hip = False
        self.hash_d2h = True

    def add(self, *parts):
        for p in parts:
            self.h.update(p if isinstance(p, bytes) else str(p).encode())
            self.h.update(b"|")


class Fn:
    """one entry of the library: records its name and status, the bytes aqg_d2h brought back, and the route words behind the entries that
    have a reporter; everything else (restype, argtypes) goes to the real ctypes function"""

    def __init__(self, lib, name, real, rec):
        object.__setattr__(self, "_s", (lib, name, real, rec))

    def __getattr__(self, k):
        return getattr(self._s[2], k)

    def __setattr__(self, k, v):
        setattr(self._s[2], k, v)

    def __call__(self, *args):
        lib, name, real, rec = self._s
        rc = real(*args)
        rec.called.add(name)
        if name in VOID:
            pass
        elif real.restype is C.c_int or real.restype is None or name in ("aqg_groupby_ngroups", "aqg_groupby_nrows", "aqg_groupby_plan"):
            rec.add(name, rc)
            if rc == 1 and real.restype is C.c_int and name not in NOT_A_STATUS:
                rec.failed_in_hip = True
        if name == "aqg_d2h" and rc == 0 and not rec.hash_d2h:
            pass
        elif name == "aqg_d2h" and rc == 0:
            rec.add(C.string_at(_int(args[1]), _int(args[3])))
        elif rc == 0 and args:
            ctx, r = args[0], rec.routes
            a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
            if name in RANK and lib.aqg_rank_last(ctx, C.byref(a), C.byref(b)) == 0:
                r["rank"] |= a.value
            elif name in JOIN and lib.aqg_join_last(ctx, C.byref(a), C.byref(b), C.byref(c)) == 0:
                r["join"] |= a.value
            elif name == "aqg_join_asof" and lib.aqg_join_asof_last(ctx, C.byref(a), C.byref(b), C.byref(c)) == 0:
                r["asof"] |= a.value
            elif name in WJ and lib.aqg_join_window_last(ctx, C.byref(a), C.byref(b), C.byref(c)) == 0:
                r["wj"] |= a.value
            elif name in SELECT and lib.aqg_select_last_routes(ctx, C.byref(a), C.byref(b)) == 0:
                r["select"] |= a.value
                rec.add("passes", b.value)
            elif name == "aqg_str_encode" and lib.aqg_str_encode_last(ctx, C.byref(a), C.byref(b)) == 0:
                r["str"] |= a.value
            elif name == "aqg_sort_rows" and lib.aqg_sort_last_passes(ctx, C.byref(a)) == 0:
                r["sort"].add("%s:%d" % ("wg" if _int(args[7]) <= cat.SORT_SMALL else "multi", min(a.value, 2)))
        return rc


class RecLib:
    def __init__(self, real, rec):
        self.__dict__["_real"], self.__dict__["_rec"], self.__dict__["_fns"] = real, rec, {}

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if not name.startswith("aqg_"):
            return f
        if name not in self._fns:
            self._fns[name] = Fn(self._real, name, f, self._rec)
        return self._fns[name]


class Env:
    def __init__(self, oracle):
        self.oracle = oracle
        self.recs = [Recorder()]
        self.dev = aquery2_amd.Device(0)
        self.dev.lib = RecLib(self.dev.lib, self.recs[0])
        self.devs = [self.dev]
        self._ranks = []

    def ranks(self, world):
        """`world` contexts on this device with an all-gather of device copies (capi.ThreadRanks), every one recorded"""
        tr = P.ThreadRanks(world, 0)
        for d in tr.devs:
            rec = Recorder()
            d.lib = RecLib(d.lib, rec)
            self.recs.append(rec)
            self.devs.append(d)
        self._ranks.append(tr)
        return tr

    def reports(self):
        out = []
        for d in self.devs:
            raw = d.lib._real
            info = P.WsInfo()
            raw.aqg_debug_ws_info(d.ctx, C.byref(info), None, 0)
            if not info.guard:
                return None
            r = P.WsReport()
            rc = raw.aqg_debug_ws_check(d.ctx, C.byref(r))
            out.append({"status": rc, "kind": r.kind, "offset": r.offset, "alloc_index": r.alloc_index, "alloc_offset": r.alloc_offset,
                        "alloc_bytes": r.alloc_bytes, "expected": r.expected, "found": r.found, "logical_bytes": info.logical_bytes})
        return out

    def close(self):
        for tr in self._ranks:
            tr.close()
        self.dev.close()


def digest_value(rec, v):
    if isinstance(v, np.ndarray):
        rec.add(v.dtype.str, v.shape, np.ascontiguousarray(v).tobytes())
    elif isinstance(v, (list, tuple)):
        for x in v:
            digest_value(rec, x)
    elif isinstance(v, np.generic):
        rec.add(v.dtype.str, v.tobytes())
    else:
        rec.add(repr(v))


def run_call(c, oracle, log):
    log.write(json.dumps({"start": c.name}) + "\n")
    log.flush()
    t0 = time.time()
    line = {"name": c.name, "status": "ok", "plan": 0}
    env = None
    try:
        env = Env(oracle)
        env.recs[0].hash_d2h = c.d2h
        ret = c.fn(env) or {}
        digest_value(env.recs[0], ret.get("out", []))
        line["plan"] = int(ret.get("plan", 0))
    except Exception as e:  # noqa: BLE001 -- reported in the log; the parent asserts on it
        line["status"] = "error"
        line["error"] = "%s: %s" % (type(e).__name__, e)
        line["traceback"] = traceback.format_exc()[-3000:]
    hip = False
    if env is not None:
        try:
            env.dev.sync()
            line["guard"] = env.reports()
        except Exception as e:  # noqa: BLE001
            line["status"], line["error"] = "error", "after the call: %s" % e
            hip = True
        recs = env.recs
        h = hashlib.sha256()
        for r in recs:
            h.update(r.h.digest())
        line["digest"] = h.hexdigest()
        line["called"] = sorted(set().union(*[r.called for r in recs]))
        routes = {k: 0 for k in ("rank", "join", "asof", "wj", "select", "str")}
        sort = set()
        for r in recs:
            for k in routes:
                routes[k] |= r.routes[k]
            sort |= r.routes["sort"]
        routes["sort"] = sorted(sort)
        line["routes"] = routes
        hip = hip or any(r.failed_in_hip for r in recs)
        try:
            env.close()
        except Exception as e:  # noqa: BLE001
            line["status"], line["error"] = "error", "closing: %s" % e
            hip = True
    line["seconds"] = round(time.time() - t0, 3)
    line["hip_failure"] = hip
    log.write(json.dumps(line) + "\n")
    log.flush()
    return not hip


def controls(log):
    """the guard finds a planted byte: in the first zone, at the very end of the tail, in the ranking bitmap.  A fresh Device each: the
    first violation is latched for good."""
    def planted(what, setup, where):
        log.write(json.dumps({"start": "control_" + what}) + "\n")
        log.flush()
        d = aquery2_amd.Device(0)
        line = {"name": "control_" + what, "status": "ok"}
        try:
            setup(d)
            before = d.debug_ws_check()
            info = d.debug_ws_info()
            addr, off, byte = where(info)
            d.memset(addr, byte, 1)
            after = d.debug_ws_check()
            again = d.debug_ws_check()
            line.update(before=before, after=after, again=again, want_offset=off, allocs=len(info["allocs"]), logical_bytes=info["logical_bytes"],
                        physical_bytes=info["physical_bytes"], rank_bm_bytes=info["rank_bm_bytes"])
        except Exception as e:  # noqa: BLE001
            line["status"], line["error"] = "error", "%s: %s\n%s" % (type(e).__name__, e, traceback.format_exc()[-2000:])
        d.close()
        log.write(json.dumps(line) + "\n")
        log.flush()

    def a_scan(d):
        x = np.arange(3 * cat.SCAN_TILE + 5, dtype=np.int32)
        assert d.scan(checker.SCAN_NAMES["mins"], x[::-1].copy()).tolist() == x[::-1].tolist()

    def a_groupby(d):
        # the all-zero ranking bitmap is taken by hint > 4096 with 64 * hint < n / 32 (make_agg_plan, groupby.hip): 8.4e6 rows at the least
        n = 8_400_007
        key = (np.arange(n, dtype=np.int64) % 4097).astype(np.int32)
        gb = d.groupby_agg([key], [checker.RED_COUNT], [key], hint=4097)
        assert gb.ngroups == 4097
        gb.destroy()
    pat = int(os.environ["AQG_WS_GUARD"], 0) & 0xFF
    planted("zone", a_scan, lambda i: (i["base"] + i["allocs"][0][0] - 256, i["allocs"][0][0] - 256, pat ^ 0x5A))
    planted("tail", a_scan, lambda i: (i["base"] + i["physical_bytes"] - 1, i["physical_bytes"] - 1, pat ^ 0x5A))
    planted("rank_bm", a_groupby, lambda i: (i["rank_bm"] + 5, 5, 0x10))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log")
    ap.add_argument("--families", default="")
    ap.add_argument("--switches", default="")
    ap.add_argument("--names", default="")
    ap.add_argument("--controls", action="store_true")
    a = ap.parse_args()
    with open(a.log, "w") as log:
        if a.controls:
            controls(log)
            log.write(json.dumps({"done": True}) + "\n")
            return 0
        oracle = checker.load_oracle()
        fams = set(filter(None, a.families.split(",")))
        names = set(filter(None, a.names.split(",")))
        for c in cat.CALLS:
            if c.switches != a.switches or (fams and c.family not in fams) or (names and c.name not in names):
                continue
            if not run_call(c, oracle, log):
                log.write(json.dumps({"stopped": c.name}) + "\n")
                return 3
        log.write(json.dumps({"done": True}) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
