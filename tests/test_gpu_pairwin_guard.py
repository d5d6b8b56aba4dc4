"""The scratch-memory guard over the pair windows' calls (tests/pairwin_scratch.py), as tests/test_gpu_scratch_guard.py holds the
catalogue's families: the child runs twice unguarded and once under AQG_WS_GUARD = 0x00, 0xFF, 0xA5, one after another, each under its
own time limit; after a child that died by a signal, ran out of time or failed inside the HIP runtime no further child is started.
Asserted: every call of every child passes its own model comparison; every guarded call's report is clean; digests, route words and plan
bits of a call are identical in all children; the call drove the entries it names."""
import json
import os
import subprocess
import sys

import pytest

import pairwin_scratch as ps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = ("0x00", "0xFF", "0xA5")
CHILD_TIMEOUT = 60


def run_child(tmp_path, tag, env_extra):
    log = str(tmp_path / ("%s.jsonl" % tag))
    env = {k: v for k, v in os.environ.items() if k != "AQG_WS_GUARD"}
    env.update(env_extra)
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pairwin_scratch_child.py"), log, "--families", ps.FAMILY],
                             capture_output=True, text=True, timeout=CHILD_TIMEOUT, env=env, cwd=ROOT)
        rc, err = out.returncode, out.stderr[-3000:]
    except subprocess.TimeoutExpired:
        rc, err = None, "time limit"
    lines = [json.loads(l) for l in open(log)] if os.path.exists(log) else []
    started = [l["start"] for l in lines if "start" in l]
    if rc is None or rc < 0 or rc == 3:
        pytest.fail("child %s ended with %r in call %r: no further child is started\n%s" % (tag, rc, started[-1] if started else None, err))
    assert rc == 0 and lines and lines[-1].get("done"), (tag, rc, err)
    return {l["name"]: l for l in lines if "name" in l}


def test_pairwin_under_the_guard(tmp_path):
    runs = {"plain": run_child(tmp_path, "plain", {}), "plain again": run_child(tmp_path, "plain_again", {})}
    for pat in PATTERNS:
        runs[pat] = run_child(tmp_path, "guard" + pat, {"AQG_WS_GUARD": pat})
    problems = []
    for c in ps.CALLS:
        base = runs["plain"].get(c.name)
        for tag, res in runs.items():
            r = res.get(c.name)
            if r is None:
                problems.append((c.name, tag, "did not run"))
                continue
            if r["status"] != "ok":
                problems.append((c.name, tag, r.get("error"), r.get("traceback", "")[-1500:]))
                continue
            if tag.startswith("plain"):
                assert r.get("guard") is None
            else:
                if not r.get("guard"):
                    problems.append((c.name, tag, "no guard report: the switch did not take"))
                for rep in r.get("guard") or []:
                    if rep["status"] != 0 or rep["kind"] != 0:
                        problems.append((c.name, tag, "guard report", rep))
            missing = set(c.entries) - set(r["called"])
            if missing:
                problems.append((c.name, tag, "entries not called", sorted(missing)))
            if base is not None and base["status"] == "ok" and (r["digest"], r["routes"], r["plan"]) != (base["digest"], base["routes"], base["plan"]):
                problems.append((c.name, tag, "differs from the unguarded run", (r["digest"][:12], base["digest"][:12])))
    assert not problems, problems
