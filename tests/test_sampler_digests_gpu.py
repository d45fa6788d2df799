"""The per-sample fp32 kernels give the bits of the commit named in tests/sampler_kernels_parent.json.

That file was recorded by tools/record_sampler_digests.py with the kernels as they stood before they were moved onto the
shared quad toolkit (csrc/quads.h) and the single spelling of the Heun step expressions: solver updates, likelihood,
noise-level evaluation, adaptive and parallel solvers, restoration, the gradient guard and the training-step elementwise
ops (the four forms of the optimizer pass included), each at CHW in {5, 1024, 1028, 3072, 65540}, B in {1, 3}, 16-byte
aligned and on a view offset by one element.  A later change to any of these kernels must not move a bit; one that means
to re-records the file and says so."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED_ROWS = 1110

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rows():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import record_sampler_digests as R
    finally:
        sys.path.pop(0)
    return R.compute(torch.device("cuda", 0))


def test_sampler_kernels_reproduce_the_parent_commits_bits(rows):
    table = json.load(open(os.path.join(ROOT, "tests", "sampler_kernels_parent.json")))
    assert len(table["parent"]) == 40
    want = [tuple(r) for r in table["rows"]]
    assert len(want) == EXPECTED_ROWS and len(rows) == EXPECTED_ROWS
    assert [r[0] for r in rows] == [r[0] for r in want]
    moved = [cid for (cid, got), (_, exp) in zip(rows, want) if got != exp]
    assert not moved, f"{len(moved)} of {len(want)} cases differ from commit {table['parent']}: {moved[:20]}"


def test_case_ids_are_unique(rows):
    assert len({r[0] for r in rows}) == len(rows)
