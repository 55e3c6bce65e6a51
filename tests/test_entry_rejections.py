"""The plan-free evaluation entry points (rae_eval_cost / _rank / _topk / _relations, the three
caller-given-queries entries and the four *_workspace_bytes functions, include/rae.h) against
tests/golden/eval_entry_rejections.json: every recorded call is refused with the recorded code
and the recorded rae_last_error() text, and every recorded shape asks for the recorded number of
workspace bytes.  oracle/gen_entry_rejections.py wrote the table and replays a line of it here.

The calls carry made-up addresses.  They are safe because each is refused before the first HIP
call; if a check were ever lost, the call would go on to launch with them.  So the module runs
only where no GPU is visible and skips itself elsewhere.

The device-side analysis entries (rae_cluster_count, rae_b3_metrics, rae_row_keys,
rae_cluster_key_count, rae_cluster_topk, rae_feature_support, rae_feature_topk and its sizing
function) are replayed the same way against tests/golden/analysis_entry_rejections.json, which
oracle/gen_analysis_rejections.py wrote; its lines with two changes pin which of two faults an
entry reports."""
import json
import os

import pytest

import gen_analysis_rejections as GA
import gen_entry_rejections as G
from conftest import GOLDEN

with open(os.path.join(GOLDEN, "eval_entry_rejections.json")) as _fh:
    TABLE = json.load(_fh)
FUNCTIONS = G.EVAL_ENTRIES + G.QUERY_ENTRIES + G.SIZERS
with open(os.path.join(GOLDEN, "analysis_entry_rejections.json")) as _fh:
    ANALYSIS = json.load(_fh)


@pytest.fixture(scope="module")
def host_lib(built_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("made-up addresses must never reach a visible GPU")
    return built_lib


def test_table_covers_every_entry():
    for fn in FUNCTIONS:
        assert sum(c["fn"] == fn for c in TABLE["rejections"]) >= 18, fn
    for fn in G.SIZERS:
        assert any(s["fn"] == fn for s in TABLE["sizes"]), fn
    assert all(c["rc"] == G.INVALID and c["msg"] for c in TABLE["rejections"])


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_refused_as_recorded(host_lib, fn):
    bad = []
    for case in TABLE["rejections"]:
        if case["fn"] != fn:
            continue
        rc, msg = G.run(host_lib, case)
        if (rc, msg) != (case["rc"], case["msg"]):
            bad.append((case, rc, msg))
    assert not bad, bad


@pytest.mark.parametrize("fn", G.SIZERS)
def test_workspace_bytes_as_recorded(host_lib, fn):
    bad = []
    for spec in TABLE["sizes"]:
        if spec["fn"] != fn:
            continue
        got = G.size_case(host_lib, spec)
        if got != spec["bytes"]:
            bad.append((spec, got))
    assert not bad, bad


def test_analysis_table_covers_every_entry():
    for fn in GA.ENTRIES:
        mine = [c for c in ANALYSIS["rejections"] if c["fn"] == fn]
        assert sum(len(c["change"]) == 1 for c in mine) >= 10, fn
        assert sum(len(c["change"]) == 2 for c in mine) >= 3, fn
    assert all(c["rc"] == G.INVALID and c["msg"] for c in ANALYSIS["rejections"])
    assert len(ANALYSIS["sizes"]) == 7 * 4 * 2 * 2


@pytest.mark.parametrize("fn", GA.ENTRIES)
def test_analysis_refused_as_recorded(host_lib, fn):
    bad = []
    for case in ANALYSIS["rejections"]:
        if case["fn"] != fn:
            continue
        rc, msg = GA.run(host_lib, case)
        if (rc, msg) != (case["rc"], case["msg"]):
            bad.append((case, rc, msg))
    assert not bad, bad


def test_analysis_workspace_bytes_as_recorded(host_lib):
    bad = [(s, got) for s in ANALYSIS["sizes"]
           for got in [GA.size_case(host_lib, s)] if got != s["bytes"]]
    assert not bad, bad
