"""tests/scratch_child.py over the calls of tests/pairwin_scratch.py: they are added to the catalogue in THIS process only, then the
child runs as it does for any family (same log, same digests, same guard report).

    python tests/pairwin_scratch_child.py LOG [--families pairwin]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import scratch_catalogue as cat  # noqa: E402
import pairwin_scratch  # noqa: E402
import scratch_child  # noqa: E402

if __name__ == "__main__":
    cat.CALLS.extend(pairwin_scratch.CALLS)
    sys.exit(scratch_child.main())
