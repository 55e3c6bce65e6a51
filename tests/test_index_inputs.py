"""The cases of tests/test_gpu_index.py, checked on the CPU: the numpy reference of the row index
(tests/_index_ref.py) passes its own invariants on every case -- every kept record once, in one
segment's range or as one mask bit; the segment rows are the kept rows minus the private ones; the
wave tasks, workgroup tasks and chunk ranges tile every non-private row once -- and every case
lands on the edge it is named for, computed from the reference.  A case that misses its edge fails
here, before a GPU is involved.  No GPU needed."""
import numpy as np
import pytest

import _index_ref as R
import test_gpu_index as S


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_case_reference_and_edge(name):
    case = S.BY_NAME[name]
    dims, refs = case.refs()
    assert dims["HA"] <= R.IDX_HMAX and dims["HW"] <= R.IDX_HMAX
    for ref in refs.values():
        R.check_invariants(ref, dims)
        assert ref["A"]["nrec"] <= dims["RA"] and ref["W"]["nrec"] <= dims["RW"]
    case.edge(dims, refs)


def test_ring_second_negatives_shorten_every_table():
    """The rebuilt slots hold fewer rows than the first build left there (stale entries behind)."""
    case = S.BY_NAME["ring_wrap_and_rebuild"]
    dims, first = case.refs()
    _, second = case.refs(S.ring_second_ids(case))
    for g in first:
        R.check_invariants(second[g], dims)
        assert second[g]["thdr"][0] < first[g]["thdr"][0]
        n1 = sum(len(np.concatenate(sg)) for sg in first[g]["A"]["segs"])
        n2 = sum(len(np.concatenate(sg)) for sg in second[g]["A"]["segs"])
        assert n2 < n1


@pytest.mark.parametrize("name", [c.name for c in S.ERROR_CASES])
def test_error_case_edges(name):
    case = S.BY_NAME[name]
    dims, refs = case.refs()
    for ref in refs.values():
        R.check_invariants(ref, dims, kcap=R.KCAP + 1)      # the overflowing partition: 8193 keys
    case.edge(dims, refs)


def test_dims_follow_the_plan_golden():
    """plan_dims against the resolved specs of tests/golden/plan_specs.json where both speak of
    the same quantity (index_window, posbits, RA / RW, TC, NVC, the descriptor stride)."""
    import json
    import os
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, "plan_specs.json")) as fh:
        specs = [e for e in json.load(fh) if e["lines"][0] == "rc 0"]
    forms = {0: "auto", 1: "off", 2: "on"}
    seen = 0
    for e in specs:
        c = e["config"]
        if c.get("lambda1") or c.get("lambda2"):
            continue
        got = {}
        for line in e["lines"]:
            kv = line.split()
            if len(kv) == 2:
                got.setdefault(kv[0], kv[1])
        G = c.get("world_size", 1)
        d = R.plan_dims(l=c["batch_size"], s=c["neg_samples"], G=G, rank=c.get("rank", 0),
                        part=c.get("dp_update", 0) == 1, window=c.get("index_window", 0),
                        n_examples=c["n_examples"], max_batch_nnz=c.get("max_batch_nnz", 0),
                        max_row_nnz=c.get("max_row_nnz", 0),
                        priv_rows=forms[c.get("priv_rows", 0)],
                        heavy_chunk=forms[c.get("heavy_chunk", 0)])
        for k in R_KEYS:
            if k in got:
                assert int(got[k]) == d[k], (e["name"], k, got[k], d[k])
                seen += 1
    assert seen > 0


R_KEYS = ("L", "RA", "RW", "HA", "HW", "index_window", "posbits", "TC", "NVC", "hch", "HF", "dcap",
          "dstride", "dnx", "priv", "privnf", "LA", "LW")
