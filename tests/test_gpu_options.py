"""One training step under every optimiser / regulariser option, the device's state against the
host references of tests/_grad_ref.py (needs an MI355X).

The shape-varying tests of this suite all train with AdaGrad, lambda = 0, alpha = 1, ext_reg and
binary features, and see the gradient only through AdaGrad's normalised step.  Here, per
(shape, option) case and for each of three batches: the generic parameters are copied into the
inducer's tensors (as a checkpoint load does), the accumulators zeroed, exactly that batch is
run, and

  cost       within COST_RTOL of the float64 oracle's (the L1 / L2 sums live here);
  AdaGrad    the gradient extracted from the state (sqrt(acc), sign of p0 - p1) has
             rho(g_gpu, g64) <= 16 max(rho(g_host32, g64), 2^-20) per tensor, and p1 is the
             AdaGrad step of that gradient to 8 * 2^-24 (|p0| + lr);
  SGD        (lr = 1) |p1 - (p0 - lr g64)| <= lr (row tolerance) + 2^-23 |p1|;
  untouched  rows whose gradient is exactly zero keep p1 bit-identical to p0 and acc == 0;
  bf16       test_gpu_fullscale.check_bf16's rule on rho: rho(gpu, exact) <= 1.25 rho(emu, exact)
             + t and rho(gpu, emu) <= 0.25 rho(emu, exact) + t, t the fp32 tolerance above (the
             AdaGrad sign rule is applied against each reference with that reference's bound);
  forms      kernel_forms_in_use() shows the intended form;
  limits     the shapes U1-U8 sit at the upper end of what plan_resolve accepts: m = r = 512
             (eight softmax slots per lane of wave 0; the split SP forward), 65 ... 128 columns
             that are no multiple of 4 (two scalar elements per lane), the largest s at
             m = r = 512, the bilinear decoders at m = 512 (bf16: M in fp32 above m = 128);
  saturated  ("-sat") the same parameters with W, Wb x 8 (x 3 at the C3 / C5 shapes) and A,
             Ab x 2: P is one-hot to 1e-4, shifted logits reach -100 ... -200 (__expf
             underflows).  There float32 autograd's W is 1.0 from float64 in rho and the
             oracle's own P (dP - sum P dP) 2.7e-5, so the truth of W / Wb is the pairwise
             form (rae_oracle.softmax_backward_pairwise), rho divides by max(rowmax |g|,
             2^-10 max |g| of the tensor), and the yardstick is the better of float32 autograd
             and a float32 numpy restatement of the kernels' centred formula; cost, AdaGrad
             step and untouched-row rules are unchanged, and everything must be finite.
             The decoder's scores stay below 20 there; "-satu" (A, Ab x 32) puts 8 ... 93 % of
             them beyond +-87 (asserted per batch), past sigmoid_softplus's linear branch.

The yardstick is the float32 host's distance from float64 at the same parameters (measured
7e-8 ... 1e-5; up to 8.8e-4 on W where P saturates), not the code under test; the factor 16 covers __expf / __logf / rcp argument
scaling (~|x| 2^-24, |x| <~ 12) and the MFMA / wave-tree summation orders, the floor 2^-20 keeps a
near-exact host vector from setting an impossible bound.  Every measured ratio
rho_gpu / max(rho_host32, 2^-20) is printed ("RATIO ..."); profiles/options_grad_check.txt keeps
the table.

The trajectory test at the end runs whole epochs (graph-captured, graph_chunk = 2) under the
regulariser with both optimisers: state carried between steps (the dense W scratch re-zeroed,
the L1 / L2 partial slots reused, SGD steps composing).
"""
import numpy as np
import pytest

import _grad_ref as G
from _grad_ref import COST_RTOL, _check_step     # the assertions of one step live there

pytestmark = pytest.mark.gpu


def _expected_forms(c):
    reg = c["l1"] != 0.0 or c["l2"] != 0.0
    want = dict(c["want"])
    want.setdefault("priv_rows", "on" if (not reg and 2 + 2 * c["s"] <= 64) else "off")
    want.setdefault("heavy_chunk", "off")
    if c["dec"] != "sp":
        want.setdefault("bil_dp", "mtile" if (c["bf16"] and c["m"] <= 128) else "strided")
    return want


def _inducer(c, dev, forms=None):
    from rae.inducer import ReconstructInducer
    data, neg1, neg2 = G.case_dataset(c)
    kf = dict(c["forms"])
    kf.update(forms or {})
    ind = ReconstructInducer(data, {"train": {}}, np.random.RandomState(2), 1, c["lr"], c["l"],
                             c["r"], c["m"], c["s"], c["l1"], c["l2"], c["opt"], "options",
                             c["dec"], False, c["ext_reg"], False, c["alpha"], device=dev,
                             graph_chunk=1, mfma_bf16=c["bf16"], kernel_forms=kf)
    ind.compile_function()
    return ind, neg1, neg2


def _one_step_states(c, dev, forms=None, per_call=False):
    """[(cost, p1, acc1)] of the three batches, each run alone from the generic parameters and
    zero accumulators; the resolved kernel forms."""
    import torch
    ind, neg1, neg2 = _inducer(c, dev, forms)
    eng = ind.engine
    named = ind.modelFunc.named_params()
    accs = dict(zip(ind.modelFunc.param_names, ind.optimizer.accumulator or []))
    p0 = G.generic_params(c)
    if not per_call:
        eng.set_epoch_negatives(neg1, neg2)
    out = []
    for b in range(G.N_BATCHES):
        for k, v in named.items():
            v.copy_(torch.as_tensor(p0[k]))
        for v in accs.values():
            v.zero_()
        if per_call:        # func['train'](batch, neg1, neg2): the per-call ABI
            cols = slice(b * c["l"], (b + 1) * c["l"])
            cost = ind.func["train"](b, neg1[:, cols], neg2[:, cols])
        else:
            eng.run(b, 1)
            torch.cuda.synchronize()
            eng.check()
            cost = float(eng.costs[b].item())
        out.append((cost, {k: v.detach().cpu().numpy().copy() for k, v in named.items()},
                    {k: v.detach().cpu().numpy().copy() for k, v in accs.items()}))
    forms_used = eng.kernel_forms_in_use()
    ind._drop_engine()
    return out, forms_used


VARIANTS = [(s, o, None, False) for s, o in G.CASES] + [
    ("S1", "O0", "on", False), ("S1", "O0", "off", False),      # private rows on / off
    ("S3", "O1", None, True), ("H1", "O4", None, True)] + [      # func['train'], the per-call ABI
    (s, o, None, False, "saturated") for s, o in G.SAT_CASES] + [     # W, Wb x 8 (3), A, Ab x 2
    (s, o, None, False, "saturated-scores") for s, o in G.SAT_SCORE_CASES]     # ... A, Ab x 32


def _vid(v):
    return (f"{v[0]}-{v[1]}" + (f"-priv_{v[2]}" if v[2] else "") + ("-percall" if v[3] else "") +
            ({"saturated": "-sat", "saturated-scores": "-satu"}[v[4]] if v[4:] else ""))


@pytest.mark.parametrize("variant", VARIANTS, ids=[_vid(v) for v in VARIANTS])
def test_one_step_state_vs_reference(built_lib, cuda_dev, variant):
    shape, option, priv, per_call = variant[:4]
    c = G.case_config(shape, option, regime=variant[4] if variant[4:] else "generic")
    forms = {"priv_rows": priv} if priv else None
    states, used = _one_step_states(c, cuda_dev, forms, per_call)
    want = _expected_forms(c)
    if priv:
        want["priv_rows"] = priv
    assert {k: used[k] for k in want} == want, used
    bad = []
    for b, (cost, p1, acc) in enumerate(states):
        _check_step(c, b, cost, p1, acc, _vid(variant), bad)
    assert not bad, "\n".join(bad)


# --------------------------------------------------------------------------------------------
# short trajectories: state carried between steps
# --------------------------------------------------------------------------------------------
def _trajectory_oracle(c, data, bf16=False):
    from test_gpu_train import _oracle_trajectory
    tr, costs = _oracle_trajectory(c["dec"], data, 2, c["m"], c["r"], c["s"], c["l"], 1,
                                   lr=c["lr"], optimizer=c["opt"], lambda1=c["l1"],
                                   lambda2=c["l2"], ext_reg=c["ext_reg"], alpha=c["alpha"],
                                   bf16=bf16)
    return costs[0], tr.params


@pytest.mark.parametrize("shape", ["S1", "B4", "H1"])
@pytest.mark.parametrize("option", ["O1", "O4"])
def test_epoch_under_options_vs_oracle(built_lib, cuda_dev, shape, option):
    """One epoch (3 steps) with learn() from the reference initialisation, graph-captured with
    graph_chunk = 2, against the oracle's trajectory under the same options at the suite's
    tolerances (costs COST_RTOL, parameters 2e-4 + 2e-3 |p|); bf16 plans by check_bf16."""
    from rae.inducer import ReconstructInducer
    from test_gpu_fullscale import check_bf16
    from test_gpu_train import _assert_params_close, _params
    c = G.case_config(shape, option)
    c["lr"] = 0.1               # a trajectory: the reference's learning rate for both optimisers
    data, _, _ = G.case_dataset(c)
    ind = ReconstructInducer(data, {"train": {}}, np.random.RandomState(2), 1, c["lr"], c["l"],
                             c["r"], c["m"], c["s"], c["l1"], c["l2"], c["opt"], "traj", c["dec"],
                             False, c["ext_reg"], False, c["alpha"], device=cuda_dev,
                             graph_chunk=2, mfma_bf16=c["bf16"])
    ind.learn(verbose=False)
    got_c, got_p = np.array(ind.epoch_costs)[0], _params(ind)
    ind._drop_engine()
    want_c, want_p = _trajectory_oracle(c, data)
    if c["bf16"]:
        emu_c, emu_p = _trajectory_oracle(c, data, bf16=True)
        check_bf16({"exact": (want_c, want_p), "emu": (emu_c, emu_p), "gpu": (got_c, got_p)},
                   None, f"{shape} {option}")
    else:
        np.testing.assert_allclose(got_c, want_c, rtol=COST_RTOL, atol=COST_RTOL)
        _assert_params_close(got_p, want_p, f"{shape} {option}")
