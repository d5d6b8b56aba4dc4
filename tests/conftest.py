import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle():
    import checker
    return checker.load_oracle()


@pytest.fixture(scope="session")
def ref_answers():
    """the real reference's answers: live where oracle/_ref is built, recorded digests everywhere (tests/golden_util.py)"""
    import checker
    import golden_util
    ra = golden_util.RefAnswers(checker.load_ref(), record=os.environ.get("AQG_RECORD_REF_DIGESTS") == "1")
    yield ra
    if ra.record:
        ra.save()

