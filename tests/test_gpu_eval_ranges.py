"""rae_eval_cost across launch rounds on an MI355X: ranges longer than one chunk
(RAE_EV_CHUNK_BIL = 2048 examples for RESCAL / hybrid, RAE_EV_CHUNK_SP = 65536 for SP), where
from the second chunk on the terms, P and the block partials are indexed chunk-locally while the
entity ids and negatives are indexed by split row, k_eval_acc adds to the running sums, the
terms of a call without terms_out live in a workspace region every chunk reuses, and
k_eval_blocksum produces more than one partial.

Reference: oracle/rae_oracle.py in float64, called in row blocks of 4096 (tests/_entry_ref.py).
Tolerances (the project's own, test_gpu_eval): cost 2e-5 max(1, |c|); terms rtol 1e-4,
atol 1e-5; each of the three sums 2e-5 max(1, |S|) against the oracle's and 1e-12 relative
against math.fsum of the call's own float32 terms; everything else is bitwise.
"""
import math

import numpy as np
import pytest

import _entry_ref as E

pytestmark = pytest.mark.gpu

TAIL = 1024 + 37
CASES = {
    "rescal-m7-r13-s3-scalar": dict(dec="rescal", m=7, r=13, s=3),
    "hybrid-m12-r20-s3-float4": dict(dec="rescal+sp", m=12, r=20, s=3),
    "sp-m8-r16-s2": dict(dec="sp", m=8, r=16, s=2),
}


def n_rows(dec):
    C = E.CHUNK[dec]
    return (C if dec == "sp" else 2 * C) + TAIL


def row_lengths(dec, seed=11):
    """Lengths 0..11, with 0, 1 and 17 in the first chunk and 64, 65 and 130 in the last."""
    N = n_rows(dec)
    lens = np.random.RandomState(seed).randint(0, 12, size=N)
    lens[[3, 4, 5]] = [0, 1, 17]
    lens[[N - 40, N - 21, N - 2]] = [64, 65, 130]
    return lens


def problem(name):
    c = CASES[name]
    return E.EvalProblem(c["dec"], c["m"], c["r"], c["s"], row_lengths(c["dec"]), n=30, d=400,
                         seed=sorted(CASES).index(name) + 20)


def seam_ranges(dec):
    C, N = E.CHUNK[dec], n_rows(dec)
    last = (C + 1000, N - C - 1000) if dec == "sp" else (2 * C - 3, 40)
    return [(C - 8, 20), (C - 1, 2), (C, 1), last, (1, N - 1)]


@pytest.fixture(scope="module", params=sorted(CASES))
def whole(request, built_lib, cuda_dev):
    """The problem on the device, the oracle's terms of every row (computed once) and the
    whole-range call with terms_out, the workspace poisoned before it."""
    prob = problem(request.param)
    dev = E.DeviceEval(built_lib, prob, cuda_dev)
    want = prob.oracle_terms()
    dev.poison()
    out, sums = dev.run(0, prob.N, terms=True)
    return request.param, prob, dev, want, out, sums


def test_whole_range_vs_oracle(whole):
    name, prob, dev, want, out, sums = whole
    assert prob.N > E.CHUNK[prob.dec] + 1024 and prob.stride == prob.N + 7
    E.check_eval(out, sums, want, prob.s, f"{name} rows [0, {prob.N})")
    got = out.cpu().numpy()
    _, want_sums = E.cost_of_terms(want, prob.s)
    for c in range(3):
        exact = math.fsum(float(x) for x in got[:, c])
        print(f"{name} sum {c}: {sums[c]!r} fsum of the terms {exact!r} oracle {want_sums[c]!r}")
        assert abs(sums[c] - exact) <= 1e-12 * abs(exact), (c, sums[c], exact)
        assert abs(sums[c] - want_sums[c]) <= E.COST_RTOL * max(1.0, abs(want_sums[c])), c


def test_seam_ranges_bitwise(whole):
    import torch
    name, prob, dev, want, out, sums = whole
    for row0, nrows in seam_ranges(prob.dec):
        assert 0 <= row0 and row0 + nrows <= prob.N
        part, psums = dev.run(row0, nrows, terms=True)
        assert torch.equal(part, out[row0:row0 + nrows]), (name, row0, nrows)
        for c in range(3):
            exact = math.fsum(float(x) for x in part[:, c].cpu().numpy())
            assert abs(psums[c] - exact) <= 1e-12 * abs(exact), (name, row0, nrows, c)


def test_sums_without_terms_poisoned_workspace(whole):
    name, prob, dev, want, out, sums = whole
    dev.poison()
    none, got = dev.run(0, prob.N, terms=False)
    assert none is None
    assert got == sums, (name, got, sums)
    row0, nrows = seam_ranges(prob.dec)[-1]
    _, with_terms = dev.run(row0, nrows, terms=True)
    dev.poison()
    _, without = dev.run(row0, nrows, terms=False)
    assert without == with_terms, (name, without, with_terms)


def test_sums_reset_by_the_first_chunk(whole):
    import torch
    name, prob, dev, want, out, sums = whole
    C = E.CHUNK[prob.dec]
    own = torch.full((3,), float("nan"), dtype=torch.float64, device=dev.dev)
    _, alone = dev.run(C - 8, 20, terms=True, sums=own)
    shared = torch.zeros(3, dtype=torch.float64, device=dev.dev)
    _, first = dev.run(0, prob.N, terms=True, sums=shared)
    _, second = dev.run(C - 8, 20, terms=True, sums=shared)
    assert first == sums and second == alone, (name, first, second, alone)
    w = want[C - 8:C + 12].sum(axis=0)
    for c in range(3):
        assert abs(second[c] - w[c]) <= E.COST_RTOL * max(1.0, abs(w[c])), (name, c)
