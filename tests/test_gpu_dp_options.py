"""The data-parallel kernel forms, one step at a time, against the host references of
tests/_grad_ref.py (needs an MI355X; one process, tests/_loopback.py moves the ranks' bytes).

tests/test_dist.py judges the data-parallel plans by whole trajectories, mostly under AdaGrad,
whose step hardly notices a per-tensor factor on the gradient -- a dense gradient taken over
K = l instead of L (k_dpart, the rank-order block sum of the update, a normaliser in the
records) would pass there.  Here G ranks with l = L / G examples each run exactly one global
batch from the generic parameters and zero accumulators, as tests/test_gpu_options.py does for
one rank, and for each of three batches

  replicated   cost, parameters and accumulators of every rank are bit-identical to rank 0's,
               and rank 0's pass _grad_ref._check_step against the references of the GLOBAL
               batch (the single-rank case at l = L): the same rules and constants as
               tests/test_gpu_options.py -- COST_RTOL, rho(g_gpu, g64) <= 16 max(rho(g_host32,
               g64), 2^-20) per tensor, the bf16 factors 1.25 / 0.25;
  partitioned  after the owners' rows are gathered (sync_rows): every rank bit-identical to
               rank 0, rank 0 bit-identical to the replicated run of the same case (costs,
               parameters, accumulators), and _check_step on rank 0;
  forms        kernel_forms_in_use() of every rank shows the forms the case asks for.

A data-parallel form differs from the single-rank step at the same global batch in summation
order only (the ranks' blocks are added in rank order), which the factor 16 already covers.
Every COST / RATIO line is printed; profiles/dp_options_grad_check.txt keeps the table (the
limit shapes U1, U2 and U4 at two ranks: profiles/limit_shapes_grad_check.txt).

k_bil_prep (the bf16 R-gradient operands laid out by a kernel after the exchange, which every
data-parallel bf16 plan runs) is also pinned at a single rank against the forward-fused layout,
and the loopback itself against the multi-process run of tests/test_dist.py.
"""
import numpy as np
import pytest

import _grad_ref as G
from _grad_ref import _check_step
from _loopback import Ranks

pytestmark = pytest.mark.gpu


def _dp_forms(c, dense, priv):
    kf = dict(c["forms"])
    if dense:
        kf["dp_dense"] = dense
    if priv:
        kf["priv_rows"] = priv
    return kf


def _dp_expected_forms(c, dense, priv, part):
    """What the plan must resolve (csrc/rae_plan.hpp): private rows by default in replicated
    plans without a regulariser and with at most 64 record slots; bf16 plans of several ranks
    lay their operands out with k_bil_prep."""
    reg = c["l1"] != 0.0 or c["l2"] != 0.0
    want = dict(c["want"])
    want["dp_update"] = "partitioned" if part else "replicated"
    want["dp_xchg"] = "collective"
    want["priv_rows"] = priv or ("on" if (not reg and not part and 2 + 2 * c["s"] <= 64) else "off")
    want.setdefault("heavy_chunk", "off")
    if dense:
        want["dp_dense"] = dense
    if c["dec"] == "sp":
        want.setdefault("sp_forward", "fused")
    else:
        want["bil_dp"] = "mtile" if (c["bf16"] and c["m"] <= 128) else "strided"
        if c["bf16"]:
            want["bil_prep"] = "kernel"
    return want


def _dp_one_step_states(c, ranks, dev, forms, part):
    """test_gpu_options._one_step_states for `ranks` ranks of the global config c: per batch the
    [(cost, p1, acc)] of every rank, each batch run alone from the generic parameters and zero
    accumulators (partitioned: read after the owners' rows are gathered); the forms per rank."""
    import torch
    from rae.inducer import ReconstructInducer
    data, neg1, neg2 = G.case_dataset(c)
    assert c["l"] % ranks == 0
    dp_update = "partitioned" if part else "replicated"

    def make(rank, exchange):
        return ReconstructInducer(data, {"train": {}}, np.random.RandomState(2), 1, c["lr"],
                                  c["l"] // ranks, c["r"], c["m"], c["s"], c["l1"], c["l2"],
                                  c["opt"], "dp_options", c["dec"], False, c["ext_reg"], False,
                                  c["alpha"], device=dev, world_size=ranks, rank=rank,
                                  exchange=exchange, graph_chunk=1, mfma_bf16=c["bf16"],
                                  kernel_forms=forms, dp_update=dp_update, index_overlap=False)
    rk = Ranks(ranks, make, forms)
    try:
        assert rk.nb == G.N_BATCHES and rk.part == part
        named = [ind.modelFunc.named_params() for ind in rk.inds]
        accs = [dict(zip(ind.modelFunc.param_names, ind.optimizer.accumulator or []))
                for ind in rk.inds]
        p0 = G.generic_params(c)
        rk.set_negatives([(neg1, neg2)] * ranks)
        out = []
        for b in range(G.N_BATCHES):
            for k in range(ranks):
                for name, v in named[k].items():
                    v.copy_(torch.as_tensor(p0[name]))
                for v in accs[k].values():
                    v.zero_()
            rk.step(b)
            if part:
                rk.sync()
            out.append([(rk.cost(k, b),
                         {n: v.detach().cpu().numpy().copy() for n, v in named[k].items()},
                         {n: v.detach().cpu().numpy().copy() for n, v in accs[k].items()})
                        for k in range(ranks)])
        if part:                        # every list the plans built fits the agreed capacities
            assert rk.lb.maxima and all(v <= rk.lb.bounds[t] for _, t, v in rk.lb.maxima)
        return out, rk.forms()
    finally:
        rk.close()


def _assert_same_state(a, b, what):
    assert np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes(), (what, "cost", a[0], b[0])
    for part_a, part_b in ((a[1], b[1]), (a[2], b[2])):
        assert part_a.keys() == part_b.keys(), what
        for k in part_a:
            np.testing.assert_array_equal(part_a[k], part_b[k], err_msg=f"{what} {k}")


@pytest.mark.parametrize("case", G.DP_CASES, ids=[G.dp_case_id(c) for c in G.DP_CASES])
def test_dp_one_step_state_vs_reference(built_lib, cuda_dev, case):
    shape, option, ranks, dense, priv, part = case
    c = G.dp_case_config(shape, option)
    forms = _dp_forms(c, dense, priv)
    tag = G.dp_case_id(case)
    bad = []
    runs = {}
    for mode in ([False, True] if part else [False]):
        states, used = _dp_one_step_states(c, ranks, cuda_dev, forms, mode)
        want = _dp_expected_forms(c, dense, priv, mode)
        for k, u in enumerate(used):
            assert {key: u.get(key) for key in want} == want, (k, mode, u)
        name = "partitioned" if mode else "replicated"
        for b, per_rank in enumerate(states):
            for k in range(1, ranks):
                _assert_same_state(per_rank[k], per_rank[0], f"{name} b{b} rank {k} vs rank 0")
            cost, p1, acc = per_rank[0]
            assert bool(acc) == (c["opt"] == "adagrad")
            _check_step(c, b, cost, p1, acc, tag if mode else tag.removesuffix("-part"), bad)
        runs[mode] = states
    if part:
        for b in range(G.N_BATCHES):
            _assert_same_state(runs[True][b][0], runs[False][b][0],
                               f"b{b} partitioned vs replicated")
    assert not bad, "\n".join(bad)


# --------------------------------------------------------------------------------------------
# k_bil_prep at a single rank
# --------------------------------------------------------------------------------------------
PREP_CASES = [("B4", "O3"), ("B5", "O3"), ("B6", "O3"), ("H3", "O3"), ("B4", "O1")]


@pytest.mark.parametrize("shape,option", PREP_CASES, ids=[f"{s}-{o}" for s, o in PREP_CASES])
def test_bil_prep_kernel_equals_fused_layout(built_lib, cuda_dev, shape, option):
    """bil_prep = kernel (k_bil_prep after the forward) against auto (the forward kernels write
    facT / pfrag themselves) at one rank: cost, parameters and accumulators bit-identical for
    each of the three batches.  Both forms store the fp32 value the record holds, rounded once
    to bf16, at the same operand position -- csrc/rae_bilinear.hpp put_fac / prep_p_fragment
    from bil_encode, bil_encode_fast and the decoder's x / y loop (fused) and bil_prep, which
    reads oX / oA1 / oA2 / oY / oP of the records (kernel) -- and feed the same k_bil_rows;
    k_bil_prep zeroes the padding (b >= L, k >= m, i >= r is never read) that the fused form
    leaves zero from plan creation.  B5: L = 40, Lp = 64; B6: m = 132 > 128."""
    from test_gpu_options import _expected_forms, _one_step_states
    c = G.case_config(shape, option)
    kern, used_k = _one_step_states(c, cuda_dev, {"bil_prep": "kernel"})
    fused, used_f = _one_step_states(c, cuda_dev, {"bil_prep": "auto"})
    want = _expected_forms(c)
    assert {k: used_k[k] for k in want} == want and {k: used_f[k] for k in want} == want
    assert used_k["bil_prep"] == "kernel" and used_f["bil_prep"] == "auto"
    bad = []
    for b in range(G.N_BATCHES):
        _assert_same_state(kern[b], fused[b], f"{shape}-{option} b{b} kernel vs fused")
        _check_step(c, b, *kern[b], f"{shape}-{option}-prep_kernel", bad)
    assert not bad, "\n".join(bad)


# --------------------------------------------------------------------------------------------
# the harness against the multi-process run
# --------------------------------------------------------------------------------------------
def test_loopback_equals_two_processes(built_lib, cuda_dev, tmp_path):
    """tests/test_dist.py's own run -- two processes, gloo, host-staged exchange, learn() -- and
    the same epochs driven through the loopback from the inducers' own initialisation and
    negative draws: costs and every parameter and accumulator bit-identical."""
    from rae.inducer import ReconstructInducer
    from test_dist import DP_SHAPE, _dataset, _launch
    _launch(["gpu", str(tmp_path), "sp", "replicated"], nproc=2)
    data, gold = _dataset()
    S = DP_SHAPE
    forms = dict(dp_dense="auto", priv_rows="auto", dp_xchg="collective")

    def make(rank, exchange):
        return ReconstructInducer(data, gold, np.random.RandomState(2), S["epochs"], 0.1, S["l"],
                                  S["r"], S["m"], S["s"], 0.0, 0.0, "adagrad", "dp", "sp", False,
                                  True, False, 1.0, device=cuda_dev, world_size=2, rank=rank,
                                  exchange=exchange, graph_chunk=1, dp_update="replicated",
                                  kernel_forms=forms, index_overlap=False)
    rk = Ranks(2, make, forms)
    try:
        costs = [[] for _ in range(2)]
        for _ in range(S["epochs"]):
            rk.set_negatives([ind.draw_epoch_negatives() for ind in rk.inds])
            for b in range(rk.nb):
                rk.step(b)
            for k, eng in enumerate(rk.engines):
                costs[k].append(eng.costs[:rk.nb].double().cpu().numpy())
        for k, ind in enumerate(rk.inds):
            z = np.load(tmp_path / f"gpu_replicated_sp_{k}.npz")
            np.testing.assert_array_equal(np.concatenate(costs[k]), z["costs"])
            for name, v in ind.modelFunc.named_params().items():
                np.testing.assert_array_equal(v.detach().cpu().double().numpy(), z[name],
                                              err_msg=name)
            acc = dict(zip(ind.modelFunc.param_names, ind.optimizer.accumulator))
            assert sorted("acc_" + n for n in acc) == sorted(f for f in z.files
                                                             if f.startswith("acc_"))
            for name, v in acc.items():
                np.testing.assert_array_equal(v.detach().cpu().numpy(), z["acc_" + name],
                                              err_msg=name)
    finally:
        rk.close()
