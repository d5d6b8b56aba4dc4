"""The scratch-memory guard over the catalogue (tests/scratch_catalogue.py, DESIGN.md "Scratch memory").  Per family of calls the child
(tests/scratch_child.py) runs twice unguarded and once under AQG_WS_GUARD = 0x00, 0xFF, 0xA5, in that order, one after another, each
under its own time limit; after a child that died by a signal or ran out of time no further child is started.  0x00 is what a fresh
arena holds and what a cleared counter looks like, 0xFF is NOROW, 0xA5 is no sentinel of the library: a buffer that a kernel reads
before anything wrote it gives a digest that moves with the pattern.

Asserted: every call of every child ends with the status the catalogue names and (unguarded child: the family's own model or oracle
comparison inside the call) passes; every guarded call's report is clean -- nothing outside its sub-allocations was written, the ranking
bitmap is all zero, no sub-allocation went past the exact capacity; digests, route words and plan bits of a call are identical in all
children -- the second unguarded one included: a call whose bytes differed between two unguarded runs could not be held to bit
equality under the guard, and there is none; the call drove the entries and took the routes and plans the catalogue says it does."""
import json
import os
import subprocess
import sys

import pytest

import scratch_catalogue as cat

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = ("0x00", "0xFF", "0xA5")
CHILD_TIMEOUT = 60            # a child takes 0.5 - 3 s on the MI355X
STOP = {"why": None}          # set by a child that was killed: nothing more is started in this process


def run_child(tmp_path, tag, env_extra, args):
    if STOP["why"]:
        pytest.fail("not started: " + STOP["why"])
    log = str(tmp_path / ("%s.jsonl" % tag))
    env = {k: v for k, v in os.environ.items() if k != "AQG_WS_GUARD" and k not in {s for v in cat.SWITCH_SETS.values() for s in v}}
    env.update(env_extra)
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scratch_child.py"), log] + args, capture_output=True, text=True,
                             timeout=CHILD_TIMEOUT, env=env, cwd=ROOT)
        rc, err = out.returncode, out.stderr[-3000:]
    except subprocess.TimeoutExpired:
        rc, err = None, "time limit"
    lines = [json.loads(l) for l in open(log)] if os.path.exists(log) else []
    started = [l["start"] for l in lines if "start" in l]
    if rc is None or rc < 0:
        STOP["why"] = "child %s %s in call %r" % (tag, "ran out of time" if rc is None else "died by signal %d" % -rc, started[-1] if started else None)
        pytest.fail(STOP["why"] + "\n" + err)
    results = {l["name"]: l for l in lines if "name" in l}
    if rc == 3:           # a call failed inside the HIP runtime (how a fault that the process survives shows): nothing more runs on this GPU
        STOP["why"] = "child %s stopped at a failure inside the HIP runtime in call %r" % (tag, started[-1] if started else None)
        pytest.fail(STOP["why"] + "\n%r\n%s" % ([r for r in results.values() if r["status"] != "ok"][:1], err))
    assert rc == 0 and lines and lines[-1].get("done"), (tag, rc, err)
    print("child %s: %d calls, %.1f s" % (tag, len(results), sum(r.get("seconds", 0) for r in results.values())))
    return results


def check_family(tmp_path, family, switches="", patterns=PATTERNS):
    calls = [c for c in cat.CALLS if c.family == family and c.switches == switches]
    assert calls
    args = ["--families", family, "--switches", switches]
    sw = cat.SWITCH_SETS[switches]
    runs = {"plain": run_child(tmp_path, "plain", sw, args), "plain again": run_child(tmp_path, "plain_again", sw, args)}
    for pat in patterns:
        runs[pat] = run_child(tmp_path, "guard" + pat, dict(sw, AQG_WS_GUARD=pat), args)
    problems = []
    for c in calls:
        base = runs["plain"].get(c.name)
        for tag, res in runs.items():
            r = res.get(c.name)
            if r is None:
                problems.append((c.name, tag, "did not run"))
                continue
            if r["status"] != "ok":
                problems.append((c.name, tag, r.get("error"), r.get("traceback", "")[-1500:]))
                continue
            if not tag.startswith("plain"):
                if not r.get("guard"):
                    problems.append((c.name, tag, "no guard report: the switch did not take"))
                for rep in r.get("guard") or []:
                    if rep["status"] != 0 or rep["kind"] != 0:
                        problems.append((c.name, tag, "guard report", rep))
            else:
                assert r.get("guard") is None
            missing = set(c.entries) - set(r["called"])
            if missing:
                problems.append((c.name, tag, "entries not called", sorted(missing)))
            for kind, want in c.expect.items():
                got = r["plan"] if kind == "plan" else r["routes"][kind]
                if (kind == "sort" and not set(want) <= set(got)) or (kind != "sort" and got & want != want):
                    problems.append((c.name, tag, "route / plan", kind, got, want))
            if base is not None and base["status"] == "ok" and (r["digest"], r["routes"], r["plan"]) != (base["digest"], base["routes"], base["plan"]):
                problems.append((c.name, tag, "differs from the unguarded run", {"digest": (r["digest"][:12], base["digest"][:12]), "routes": (r["routes"], base["routes"]),
                                                                                 "plan": (r["plan"], base["plan"])}))
    assert not problems, problems


DEFAULT_FAMILIES = sorted({c.family for c in cat.CALLS if c.switches == ""})


@pytest.mark.parametrize("family", DEFAULT_FAMILIES)
def test_family_under_the_guard(tmp_path, family):
    check_family(tmp_path, family)


@pytest.mark.parametrize("switches", sorted(s for s in cat.SWITCH_SETS if s))
def test_forced_plans_under_the_guard(tmp_path, switches):
    """plans the default thresholds do not reach: the switch sets of tests/test_gpu_plans.py, each with an unguarded child of its own to
    compare with, pattern 0xA5 only"""
    for family in sorted({c.family for c in cat.CALLS if c.switches == switches}):
        check_family(tmp_path, family, switches, patterns=("0xA5",))


@pytest.mark.parametrize("pattern", PATTERNS)
def test_positive_controls(tmp_path, pattern):
    """no faulty kernel needed: one byte written with aqg_memset into the first red zone, into the last byte of the tail, into the ranking
    bitmap after a group-by that took it -- the check reports exactly that byte, was clean before, and keeps the report"""
    res = run_child(tmp_path, "controls" + pattern, {"AQG_WS_GUARD": pattern}, ["--controls"])
    for what, kind in (("zone", 1), ("tail", 3), ("rank_bm", 4)):
        r = res["control_" + what]
        assert r["status"] == "ok", r
        assert r["before"]["kind"] == 0, (what, r["before"])
        assert r["after"]["kind"] == kind and r["after"]["offset"] == r["want_offset"], (what, r["after"], r["want_offset"])
        assert r["again"] == r["after"], what
        if what != "rank_bm":
            assert r["after"]["expected"] == int(pattern, 0) and r["after"]["found"] == int(pattern, 0) ^ 0x5A
            assert r["allocs"] >= 1 and r["logical_bytes"] % 256 == 0 and r["physical_bytes"] > r["logical_bytes"]
        else:
            assert r["rank_bm_bytes"] > 0 and r["after"]["found"] == 0x10
