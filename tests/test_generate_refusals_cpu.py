"""What generate refuses before anything is loaded, pinned message by message: one valid option set, every single
perturbation of it below and every pair of them, replayed against `generate._validate` and compared with the recorded
tests/golden/generate_refusals.json (null = accepted).  The table was recorded from the `_check_*` calls in generate()'s
order before they were gathered into `_validate`.  After adding a flag: add its perturbations here, print `_rows()` as
{"cases": [...], "message": ...} rows and review the diff of the table by hand."""
import inspect
import itertools
import json
import os

import pytest

from tinyedm_amd import generate as G

BASE = {"init_dir": "d", "image_size": 32, "num_steps": 8}
PERTURBATIONS = [
    ("init_dir", None), ("start_step", 3), ("start_step", 8), ("start_step", True), ("mask_box", (1, 1, 5, 5)),
    ("mask_box", (5, 1, 1, 5)), ("invert_to", "o.pt"), ("likelihood_to", "o.json"), ("num_probes", 2),
    ("dequantize", True), ("solver", "dpmpp"), ("S_churn", 5), ("network_dtype", "bf16"), ("restore_scale", 4),
    ("restore_scale", 3), ("restore_gray", True), ("save_degraded", "deg"), ("restore_report", "r.json"),
    ("dps_scale", 1.0), ("dps_scale", -1), ("blur_std", 1.0), ("blur_radius", 5), ("measurement_noise", 0.1),
    ("labels_to", "l.json"), ("guided", True),
]


def _name(p) -> str:
    return f"{p[0]}={p[1]!r}"


def _baseline() -> dict:
    """_validate's options at generate()'s own defaults, with BASE on top"""
    defaults = {k: p.default for k, p in inspect.signature(G.generate).parameters.items()}
    return {**{k: defaults.get(k, False) for k in inspect.signature(G._validate).parameters}, **BASE}


def _rows():
    """every single perturbation, then every pair that sets two different options: (names, options)"""
    combos = [(p,) for p in PERTURBATIONS] + [c for c in itertools.combinations(PERTURBATIONS, 2) if c[0][0] != c[1][0]]
    return [([_name(p) for p in c], {**_baseline(), **dict(c)}) for c in combos]


def test_validate_refuses_as_recorded(golden_dir):
    with open(os.path.join(golden_dir, "generate_refusals.json")) as f:
        recorded = {tuple(r["cases"]): r["message"] for r in json.load(f)}
    rows = _rows()
    assert set(recorded) == {tuple(names) for names, _ in rows}
    wrong = []
    for names, options in rows:
        try:
            G._validate(**options)
            got = None
        except ValueError as e:
            got = str(e)
        if got != recorded[tuple(names)]:
            wrong.append((names, recorded[tuple(names)], got))
    assert not wrong, wrong[:5]


def test_validate_accepts_the_baseline_and_names_the_tasks():
    assert G._validate(**_baseline()) == (False, False)
    assert G._validate(**{**_baseline(), "restore_scale": 4}) == (False, True)
    assert G._validate(**{**_baseline(), "dps_scale": 1.0, "blur_std": 1.0, "network_dtype": "bf16"}) == (True, True)


def test_rank_path():
    assert G._rank_path("a/b.json", 0, 1) == "a/b.json"
    assert G._rank_path("a/b.json", 3, 4) == "a/b.rank3.json"
