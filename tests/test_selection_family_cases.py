"""tests/selection_family_cases.py on the CPU: every generated case has one answer per question (no model flags a slot), the three
numpy models agree on it bit for bit, and the shapes are the ones the GPU test (tests/test_gpu_selection_family.py) is there for."""
import numpy as np

import selection_family_cases as sf
from selection_family_cases import ROUTE_GROUP, ROUTE_SMALL, ROUTE_SPLIT, SMALL_CAP, SPLIT_CHUNK, TILE


def test_models_agree_and_flag_nothing():
    seen = 0
    for name, dt, counts, x in sf.generate():
        assert x.dtype == dt and len(x) == sum(counts) <= 20_000, (name, len(x))
        assert not np.isnan(x.astype(np.float64)).any() and np.all(x != 0), (name, dt)
        for question, answers in sf.models(x, counts).items():
            (a, fa), (b, fb) = answers.values()
            assert not fa.any() and not fb.any(), (name, dt, question)
            assert a.dtype == b.dtype == dt and a.tobytes() == b.tobytes(), (name, dt, question, list(answers))
        seen += 1
    assert seen == len(sf.CASES) * len(sf.DTYPES)


def test_slices_start_off_the_boundary():
    off = sf.offsets(sf.CASES["misaligned starts"])[:-1]
    for dt in sf.DTYPES:
        v = 16 // dt.itemsize
        assert set(range(1, min(v, 4))) <= set(int(o) % v for o in off), dt
    # ... and long ones too: a slice that the GROUP and SPLIT routes read with 16-byte loads in the middle
    assert any(o % 16 in (1, 2, 3) and c > 512 for o, c in zip(off, sf.CASES["misaligned starts"]))


def test_slices_shorter_than_a_vector():
    counts = sf.CASES["shorter than a vector"]
    for dt in sf.DTYPES:
        assert set(range(1, 16 // dt.itemsize)) <= set(counts), dt


def test_chunk_lengths():
    lens = sorted(max(c) for name, c in sf.CASES.items() if name.startswith("chunk"))
    assert lens == [SPLIT_CHUNK - 1, SPLIT_CHUNK, SPLIT_CHUNK + 1, 2 * SPLIT_CHUNK + 1]
    for name, c in sf.CASES.items():
        if name.startswith("chunk"):
            assert sf.expected_routes(c, "split") == ROUTE_SPLIT and c[0] % 16 != 0, name


def test_a_small_group_straddles_a_tile_border():
    counts = sf.CASES["tile border"]
    off = sf.offsets(counts)
    hits = [g for g in range(len(counts) - 1)
            if counts[g] <= SMALL_CAP < counts[g + 1] and off[g] // TILE != (off[g + 1] - 1) // TILE]
    assert hits and any(c <= SMALL_CAP for c in counts[hits[0] + 2:]), "a SMALL group over the border, a longer one, SMALL groups behind it"
    assert sf.expected_routes(counts, "small") == ROUTE_SMALL | ROUTE_GROUP
    assert sf.expected_routes(counts, "small+split") == ROUTE_SMALL | ROUTE_SPLIT
    assert sf.expected_routes(counts, "group") == ROUTE_GROUP and sf.expected_routes(counts, "split") == ROUTE_SPLIT
