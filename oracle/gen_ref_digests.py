#!/usr/bin/env python3
"""Generate tests/golden/ref_digests.json: the digests of the REAL reference library's answers to every question the host-only
reference-parity tests ask (tests/test_oracle_vs_ref.py, tests/test_oracle_extremes.py, tests/test_oracle_keys.py,
tests/test_egress_text.py), so that those
tests check the oracle where the reference is not built.

Runs only where oracle/_ref/libaqref.so exists (`make -C oracle ref` where the reference sources are mounted); the tests run in
recording mode, asking the live library and checking the oracle against it as they go.
    python oracle/gen_ref_digests.py
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libaqref.so")):
    sys.exit("oracle/_ref/libaqref.so missing: run `make -C oracle ref` where the reference sources are mounted")
tests = ["tests/test_oracle_vs_ref.py", "tests/test_oracle_extremes.py", "tests/test_oracle_keys.py", "tests/test_egress_text.py"]
sys.exit(subprocess.call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", *tests], cwd=ROOT,
                         env=dict(os.environ, AQG_RECORD_REF_DIGESTS="1")))
