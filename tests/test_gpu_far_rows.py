"""Row addressing past 2^31 (and 2^32) elements: one training step per batch on parameter tables
of 8 ... 32 GiB whose only live rows are those of a small case of tests/_grad_ref.py (needs an
MI355X).

Relabelling invariance with inert padding (tests/_far_rows.py): the case's entity ids (A, Ab) or
feature ids (W) are sent through far_map onto rows around the element offsets 2^29, 2^30, 2^31
(byte offsets 2^31, 2^32, 2^33; one case 2^32 elements), every other row holds a padding value.
Per batch, each run alone from the generic parameters and zero accumulators:

  (i)    the touched rows gathered back into compact arrays, the dense tensors and the cost go
         through _grad_ref._check_step unchanged: the float64 references, factor 16 / floor
         2^-20, the bf16 1.25 / 0.25 rule -- no new tolerance;
  (ii)   the same case run compact on the device in the same test: cost, every mapped row of the
         parameters and accumulators and every dense tensor are BITWISE equal (DESIGN.md
         section 3: the order of every sum is a function of the records, not of the row ids;
         the CSR keeps the compact case's feature order within an example);
  (iii)  the padding check: the rows that differ from the padding value are mapped rows, the
         rows with a non-zero accumulator are rows the batch touches;
  (iv)   kernel_forms_in_use() shows the case's forms.

Padding: a non-zero constant (A 0.25, Ab -0.5, W 0.125) without a regulariser -- a read of a
padding row would show; exactly 0 for W under a regulariser: k_dense_w computes g = 0 there
(sgnf(0) = 0), W stays bit-zero with a zero accumulator and the cost's L1 / L2 sums are the
compact case's.  tests/test_far_rows_host.py shows on the CPU that a row product in int32 or
uint32, or a byte offset modulo 2^32, reads something else for every mapped row it moves.

Each test allocates its tables (need printed and in the skip message), frees them before it
returns, and skips only when the device has less free memory than its need plus 4 GiB.
"""
import gc

import numpy as np
import pytest
import scipy.sparse as sp

import _far_rows as F
import _grad_ref as G
from _grad_ref import _check_step
from test_far_rows_host import A_CASES, W_CASES, case_counts

pytestmark = pytest.mark.gpu

GIB = 1 << 30
PADS = {"A": 0.25, "Ab": -0.5, "W": 0.125}
TABLE_OF = {"A": "A", "Ab": "A", "W": "W"}     # Ab shares A's map

# (shape, option, far tables, top, forms): the issue's list
CASES = ([(s, o, ("A",), 2 ** 31, None) for s, o in A_CASES] +
         [(s, o, ("W",), 2 ** 31, None) for s, o in W_CASES] +
         [("S1", "O0", ("A", "W"), 2 ** 31, {"priv_rows": "on"}),
          ("S3", "O3", ("A",), 2 ** 32, None)])


def _cid(case):
    return f"{case[0]}-{case[1]}-{'+'.join(case[2])}far" + ("-2e32" if case[3] == 2 ** 32 else "")


class _Split:
    """A train split whose CSR keeps the order it is given (DatasetSplit sorts the column
    indices of a row; a non-monotone map would then reorder an example's features, and with
    them the encoder's sum)."""

    def __init__(self, a1, a2, X):
        self.args1 = np.ascontiguousarray(a1, dtype=np.int32)
        self.args2 = np.ascontiguousarray(a2, dtype=np.int32)
        self.xFeats = X


def _maps(c, far, top):
    """{table: FarMap or None} and the per-batch record counts of both tables."""
    ca, cw = case_counts(c)
    fa = F.far_map(ca, c["r"], top) if "A" in far else None
    fw = F.far_map(cw, c["m"], top) if "W" in far else None
    return {"A": fa, "W": fw}, {"A": ca, "W": cw}


def need_bytes(c, fms):
    """Device bytes of a far run: the far tables, their accumulators, the dense-W scratch of a
    regulariser plan, 1 GiB for the padding check's temporaries and 1 GiB for the rest."""
    per_row = {"A": 4 * (c["r"] + 1), "W": 4 * c["m"]}
    total = 2 * GIB
    for t, fm in fms.items():
        if fm is None:
            continue
        b = fm.n_far * per_row[t]
        total += b * (2 if c["opt"] == "adagrad" else 1)
        if t == "W" and (c["l1"] or c["l2"]):
            total += b
    return total


def _free_device():
    import torch
    gc.collect()
    torch.cuda.empty_cache()


class _FarRun:
    """One engine of case c on tables laid out by fms ({table: FarMap or None = compact}), its
    model built from device tensors.  ranks > 1: rank `rank` of a data-parallel plan whose global
    batch is c["l"]."""

    def __init__(self, c, dev, fms, forms, ranks=1, rank=0, exchange=None, dp_update="replicated",
                 pads=None, problem=None):
        from rae.engine import TrainEngine
        self.c, self.fms = c, fms
        if problem is None:         # the case's own; else dict(p0, a1, a2, X, neg1, neg2)
            data, neg1, neg2 = G.case_dataset(c)
            xs = data.split["train"]
            problem = dict(p0=G.generic_params(c), a1=xs.args1, a2=xs.args2, X=xs.xFeats,
                           neg1=neg1, neg2=neg2)
        self.p0 = problem["p0"]
        neg1, neg2 = problem["neg1"], problem["neg2"]
        self.reg = bool(c["l1"] or c["l2"])
        ident = {"A": np.arange(len(self.p0["A"]), dtype=np.int64),
                 "W": np.arange(c["d"], dtype=np.int64)}
        self.rows = rows = {t: (fms[t].rows if fms[t] is not None else ident[t]) for t in ident}
        size = {t: (fms[t].n_far if fms[t] is not None else len(ident[t])) for t in ident}
        self.pads = dict(PADS, W=0.0 if self.reg else PADS["W"])
        self.pads.update(pads or {})
        self.named, self.acc = F.far_tensors(
            self.p0, {k: rows[t] for k, t in TABLE_OF.items()},
            {k: size[t] for k, t in TABLE_OF.items()}, self.pads, dev, c["opt"] == "adagrad")
        model = F.FarModel(c["dec"], c["m"], c["r"], c["s"], c["l"] // ranks, size["A"], c["alpha"],
                           c["ext_reg"], self.named)
        opt = F.FarOptimizer(c["opt"], [self.acc[k] for k in model.param_names] if self.acc else None)
        X = problem["X"]
        Xf = sp.csr_matrix((X.data, rows["W"][X.indices].astype(np.int64), X.indptr),
                           shape=(X.shape[0], size["W"]))
        split = _Split(rows["A"][problem["a1"]], rows["A"][problem["a2"]], Xf)
        self.negs = (rows["A"][neg1].astype(np.int32), rows["A"][neg2].astype(np.int32))
        kf = dict(c["forms"])
        kf.update(forms or {})
        self.kernel_forms = kf
        more = {} if ranks == 1 else dict(world_size=ranks, rank=rank, exchange=exchange,
                                          dp_update=dp_update, index_overlap=False)
        self.eng = TrainEngine(model, opt, split, learning_rate=c["lr"], lambda1=c["l1"],
                               lambda2=c["l2"], graph_chunk=1, device=dev, mfma_bf16=c["bf16"],
                               kernel_forms=kf, **more)

    def reset(self):
        """The generic parameters in every mapped row, zero accumulators there."""
        import torch
        for k, v in self.named.items():
            if k in TABLE_OF:
                F.scatter_rows(v, self.rows[TABLE_OF[k]], self.p0[k])
                if self.acc:
                    F.scatter_rows(self.acc[k], self.rows[TABLE_OF[k]], 0.0)
            else:
                v.copy_(torch.as_tensor(self.p0[k]))
                if self.acc:
                    self.acc[k].zero_()

    def state(self):
        """(parameters, accumulators) as compact arrays."""
        def pull(d):
            return {k: (F.gather_rows(v, self.rows[TABLE_OF[k]]) if k in TABLE_OF else
                        v.detach().cpu().numpy().copy()) for k, v in d.items()}
        return pull(self.named), pull(self.acc or {})

    def padding(self, b, counts, tag):
        """(iii) the padding rows still hold the padding value, and only rows batch b touches
        have an accumulator (under a regulariser every mapped W row has a gradient)."""
        viol = []
        for k, t in TABLE_OF.items():
            if self.fms[t] is None:
                continue
            rows = self.rows[t]
            bad = F.padding_violations(self.named[k], self.pads[k], rows)
            if bad.size:
                viol.append(f"{tag} b{b} {k}: {bad.size} padding rows changed, first {bad[:4]}")
            if self.acc:
                touched = rows if (t == "W" and self.reg) else rows[counts[t][b] > 0]
                bad = F.padding_violations(self.acc[k], 0.0, touched)
                if bad.size:
                    viol.append(f"{tag} b{b} acc {k}: {bad.size} untouched rows are not zero, "
                                f"first {bad[:4]}")
        return viol

    def close(self):
        if self.eng is not None:
            self.eng.close()
        self.eng = self.named = self.acc = None
        _free_device()


def _run(c, dev, fms, counts, forms, tag):
    """The three batches of case c, each alone from the generic parameters and zero
    accumulators.  Returns ([(cost, p1, acc)] with compact arrays, kernel forms, padding
    violations)."""
    import torch
    run = _FarRun(c, dev, fms, forms)
    out, viol = [], []
    try:
        eng = run.eng
        eng.set_epoch_negatives(*run.negs)
        for b in range(G.N_BATCHES):
            run.reset()
            eng.run(b, 1)
            torch.cuda.synchronize()
            eng.check()
            out.append((float(eng.costs[b].item()),) + run.state())
            viol += run.padding(b, counts, tag)
        used = eng.kernel_forms_in_use()
    finally:
        del eng
        run.close()
    return out, used, viol


def _bitwise(far, compact):
    """Names of what differs between two runs' states (cost, parameters, accumulators)."""
    diff = []
    for b, ((cf, pf, af), (cc, pc, ac)) in enumerate(zip(far, compact)):
        if np.float32(cf).tobytes() != np.float32(cc).tobytes():
            diff.append(f"b{b} cost {cf!r} != {cc!r}")
        for what, x, y in (("p", pf, pc), ("acc", af, ac)):
            for k in x:
                if x[k].tobytes() != y[k].tobytes():
                    ne = np.nonzero((x[k] != y[k]).reshape(x[k].shape[0], -1).any(axis=1))[0]
                    diff.append(f"b{b} {what} {k}: {ne.size} rows differ, first {ne[:4]}")
    return diff


def _skip_unless_fits(need):
    import torch
    free, _ = torch.cuda.mem_get_info()
    print(f"NEED {need / GIB:.1f} GiB, free {free / GIB:.1f} GiB")
    if free < need + 4 * GIB:
        pytest.skip(f"needs {need / GIB:.1f} GiB of device memory plus 4 GiB; "
                    f"{free / GIB:.1f} GiB are free")


@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", CASES, ids=[_cid(x) for x in CASES])
def test_far_rows_one_step(built_lib, cuda_dev, case):
    from test_gpu_options import _expected_forms
    shape, option, far, top, forms = case
    c = G.case_config(shape, option)
    tag = _cid(case)
    fms, counts = _maps(c, far, top)
    for t in far:
        fm = fms[t]
        assert not F.check_map(fm, counts[t])
        assert fm.n_far * fm.width > top
        if c["hot"] and t == "A":       # the >= 256-record row lies past 2^31 elements
            for b in range(G.N_BATCHES):
                hot = np.nonzero(counts[t][b] >= F.HOT)[0]
                assert np.any(fm.rows[hot] * fm.width >= 2 ** 31)
    need = need_bytes(c, fms)
    _skip_unless_fits(need)
    seams = " ".join(f"{t}@2^{S.bit_length() - 1}:{fms[t].rows_at(S)}" for t in far
                     for S in fms[t].seams)
    print(f"FAR {tag} bytes {need - 2 * GIB} rows " +
          " ".join(f"{t}:{fms[t].n_far}x{fms[t].width}" for t in far) + f" mapped {seams}")
    compact, used_c, _ = _run(c, cuda_dev, {"A": None, "W": None}, counts, forms, tag + "/compact")
    states, used, viol = _run(c, cuda_dev, fms, counts, forms, tag)
    want = _expected_forms(c)
    want.update(forms or {})
    assert {k: used[k] for k in want} == want, used                       # (iv)
    assert used == used_c
    bad = []
    for b, (cost, p1, acc) in enumerate(states):                          # (i)
        _check_step(c, b, cost, p1, acc, tag, bad)
    diff = _bitwise(states, compact)                                      # (ii)
    print(f"BITWISE {tag} {'equal' if not diff else 'DIFFERS: ' + '; '.join(diff)}")
    print(f"PADDING {tag} {'clean' if not viol else '; '.join(viol)}")
    assert not bad, "\n".join(bad)
    assert not viol, "\n".join(viol)                                      # (iii)
    assert not diff, "\n".join(diff)


# --------------------------------------------------------------------------------------------
# the partitioned update at two ranks, both replicas far
# --------------------------------------------------------------------------------------------
# from _grad_ref.DP_CASES: S1 under O0 with the private rows on (the compact privc wave and its
# e * r), under O3 with them off
DP_FAR = [("S1", "O0", 2, "partials", "on", True), ("S1", "O3", 2, "partials", "off", True)]
assert all(x in G.DP_CASES for x in DP_FAR)


def _dp_run(c, dev, fms, counts, forms, ranks, tag):
    """_run for `ranks` ranks of the partitioned update in one process (tests/_loopback.py):
    per batch the states of every rank after the owners' rows are gathered."""
    from _loopback import Ranks
    runs = []

    def make(rank, exchange):
        runs.append(_FarRun(c, dev, fms, forms, ranks, rank, exchange, "partitioned"))
        return runs[-1].eng
    rk = None
    out, viol = [], []
    try:
        rk = Ranks(ranks, make, forms)
        assert rk.nb == G.N_BATCHES and rk.part and not rk.inds
        rk.set_negatives([r.negs for r in runs])
        for b in range(G.N_BATCHES):
            for r in runs:
                r.reset()
            rk.step(b)
            rk.sync()
            out.append([(rk.cost(k, b),) + r.state() for k, r in enumerate(runs)])
            for k, r in enumerate(runs):
                viol += r.padding(b, counts, f"{tag} rank {k}")
        assert rk.lb.maxima and all(v <= rk.lb.bounds[t] for _, t, v in rk.lb.maxima)
        used = rk.forms()
    finally:
        for r in runs:
            r.eng = None if rk is not None else r.eng      # Ranks.close() closes its engines
        if rk is not None:
            rk.close()
        del rk
        for r in runs:
            r.close()
    return out, used, viol


@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", DP_FAR, ids=[G.dp_case_id(x) + "-Afar" for x in DP_FAR])
def test_far_rows_partitioned_two_ranks(built_lib, cuda_dev, case):
    """k_build_dplists (n_far is far beyond its LDS bitmap: the hash pass), rae_dp_pack_at /
    rae_dp_unpack_at, the forward and the partitioned update on far A tables of both ranks:
    checks (i) - (iii) of this module on rank 0, all ranks bit-identical after the gather."""
    from test_gpu_dp_options import _assert_same_state, _dp_expected_forms, _dp_forms
    shape, option, ranks, dense, priv, part = case
    c = G.dp_case_config(shape, option)
    tag = G.dp_case_id(case) + "-Afar"
    forms = _dp_forms(c, dense, priv)
    fms, counts = _maps(c, ("A",), 2 ** 31)
    assert not F.check_map(fms["A"], counts["A"])
    need = ranks * (need_bytes(c, fms) - 2 * GIB) + 2 * GIB
    _skip_unless_fits(need)
    print(f"FAR {tag} bytes {need - 2 * GIB} rows A:{fms['A'].n_far}x{fms['A'].width} x {ranks} "
          "ranks mapped " + " ".join(f"A@2^{S.bit_length() - 1}:{fms['A'].rows_at(S)}"
                                     for S in fms["A"].seams))
    compact, used_c, _ = _dp_run(c, cuda_dev, {"A": None, "W": None}, counts, forms, ranks,
                                 tag + "/compact")
    states, used, viol = _dp_run(c, cuda_dev, fms, counts, forms, ranks, tag)
    want = _dp_expected_forms(c, dense, priv, True)
    for k, u in enumerate(used):
        assert {key: u.get(key) for key in want} == want, (k, u)
    assert used == used_c
    bad = []
    for b, per_rank in enumerate(states):
        for k in range(1, ranks):
            _assert_same_state(per_rank[k], per_rank[0], f"b{b} rank {k} vs rank 0")
        _check_step(c, b, *per_rank[0], tag, bad)
    diff = _bitwise([s[0] for s in states], [s[0] for s in compact])
    print(f"BITWISE {tag} {'equal' if not diff else 'DIFFERS: ' + '; '.join(diff)}")
    print(f"PADDING {tag} {'clean' if not viol else '; '.join(viol)}")
    assert not bad, "\n".join(bad)
    assert not viol, "\n".join(viol)
    assert not diff, "\n".join(diff)


# --------------------------------------------------------------------------------------------
# the plan-free entries on far tables
# --------------------------------------------------------------------------------------------
RANK_ROWS = 100             # 200 queries: 2 n r nq is about 1e12 flop at n_far = 10.7 M
TOP = 10
# the compact vocabulary of the entries' case: the first RANK_N entity rows of the shape's generic
# parameters, ids taken modulo RANK_N.  Among the case's own 20 000 entities intervals() leaves
# 53 % of the float64 reference's queries open (widest 5); among 1000, 5 % (S1) and 3.5 % (B1),
# widest 1 and 2: within _rank_ref.MAX_AMBIGUOUS / MAX_WIDTH as they are
RANK_N = 1000


def _padding_bias(c, p64, X, e1, e2, n_pad):
    """B for the padding rows A = 0, Ab = -B of the ranking entries, from the float64 reference
    alone: a padding entity scores c - B for a query (q, c); B puts that below the true score
    and every compact entity's score by more than intervals' tolerance, and the padding's share
    of the log-sum-exp below TERM_ATOL / 100.  Returns (B, reference dict); both asserted."""
    import _rank_ref as R
    q, cc, u, true = R.queries64(c["dec"], p64, X, e1, e2)
    g = R.scores64(q, cc, p64["A"], p64["Ab"])
    lo, hi = R.intervals(g, u, true)
    R.assert_cap(lo, hi, f"{c['shape']} compact reference")    # MAX_AMBIGUOUS / MAX_WIDTH as they are
    lse = R.lse64(g, true)
    floor = np.minimum(u, g.min(axis=-1))
    B = float(np.ceil(max((cc - floor).max(), (cc - lse).max() + np.log(n_pad)) + 32.0))
    pad = cc - B
    tol = R.TERM_ATOL + R.TERM_RTOL * np.maximum(np.maximum(np.abs(u), np.abs(g).max(axis=-1)),
                                                 np.abs(pad))
    assert np.all(floor - pad > tol), (B, (floor - pad).min())
    share = n_pad * np.exp(pad - lse)           # d lse <= log1p(share) <= share
    assert share.max() < R.TERM_ATOL / 100, (B, share.max())
    E = (c["r"] + 3) * 2.0 ** -24 * (np.einsum("btr,er->bte", np.abs(q), np.abs(p64["A"])) +
                                     np.abs(cc)[..., None] + np.abs(p64["Ab"])).max(axis=-1)
    return B, dict(q=q, c=cc, u=u, true=true, lo=lo, hi=hi, lse=lse,
                   lse_bound=E + R.TERM_ATOL + R.TERM_RTOL * np.abs(lse) + share)


def _entries(run, c, e1, e2, neg1, neg2, Q, add, skip):
    """Every plan-free entry on one engine; ids as the engine's tables number them."""
    import torch
    eng, split, N = run.eng, run.eng.split, run.eng.split.N
    ev = eng.evaluate(split, 0, N, neg1, neg2, terms=True)
    out = dict(terms=ev.terms.cpu().numpy(), sums=np.array(ev.sums), cost=ev.cost)
    rk = eng.rank(split, 0, RANK_ROWS, ks=(1, 10, 100), per_query=True)
    out.update(greater=rk.greater.cpu().numpy(), equal=rk.equal.cpu().numpy(),
               target=rk.target.cpu().numpy(), lse=rk.lse.cpu().numpy(),
               ranks=(rk.mrr, rk.mean_rank, rk.hits))
    ents, sc = eng.predict_arguments(split, 0, RANK_ROWS, top=TOP)
    out.update(arg_ents=ents.cpu().numpy(), arg_scores=sc.cpu().numpy())
    ents, sc = eng.predict_arguments(split, 0, RANK_ROWS, top=TOP, skip_true=True)
    out.update(argx_ents=ents.cpu().numpy(), argx_scores=sc.cpu().numpy())
    ents, sc = eng.topk_entities(Q, TOP, add=add, skip=skip)
    out.update(q_ents=ents.cpu().numpy(), q_scores=sc.cpu().numpy())
    out["psi"] = eng.relation_scores(e1, e2).cpu().numpy().copy()
    psi, joint, ld, lj = eng.eval_relations(split, 0, N)
    out.update(rel_psi=psi.cpu().numpy(), rel_joint=joint.cpu().numpy(),
               rel_dec=ld.cpu().numpy(), rel_joint_labels=lj.cpu().numpy())
    lab, pr = eng.label(split, 0, N, probs=True)
    out.update(labels=lab.cpu().numpy(), probs=pr.cpu().numpy())
    torch.cuda.synchronize()
    return out


@pytest.mark.timeout(300)
@pytest.mark.parametrize("shape", ["S1", "B1"])
def test_far_rows_entries(built_lib, cuda_dev, shape):
    """rae_eval_cost, rae_eval_rank, rae_eval_topk, rae_topk_queries, rae_relation_scores,
    rae_eval_relations and rae_label with A, Ab and W far (sp at S1's shape, rescal at B1's).
    Padding rows: A = 0, Ab = -B, W = 0.125; B from _padding_bias.  Everything that does not sum
    over all entities is bitwise equal to the compact engine's (entity lists through the map);
    the ranking counts, hits and ranks are equal exactly, the log-sum-exp is within test_gpu_rank's
    bound of float64; the terms are within test_gpu_eval's TERM_RTOL / TERM_ATOL of float64."""
    from test_gpu_eval import _check, _oracle
    c = G.case_config(shape, "O3")
    tag = f"{shape}-entries-A+Wfar"
    data, neg1, neg2 = G.case_dataset(c)
    xs = data.split["train"]
    p0 = dict(G.generic_params(c))
    p0["A"], p0["Ab"] = p0["A"][:RANK_N], p0["Ab"][:RANK_N]
    prob = dict(p0=p0, a1=xs.args1 % RANK_N, a2=xs.args2 % RANK_N, X=xs.xFeats,
                neg1=neg1 % RANK_N, neg2=neg2 % RANK_N)
    ca = np.bincount(np.concatenate([prob["a1"], prob["a2"], prob["neg1"].ravel(),
                                     prob["neg2"].ravel()]), minlength=RANK_N)[None, :]
    cw = np.bincount(xs.xFeats.indices, minlength=c["d"])[None, :]
    fms = {"A": F.far_map(ca, c["r"]), "W": F.far_map(cw, c["m"])}
    assert not F.check_map(fms["A"], ca) and not F.check_map(fms["W"], cw)
    need = need_bytes(c, fms) + GIB             # + the ranking / top-k workspaces
    _skip_unless_fits(need)
    print(f"FAR {tag} bytes {need - 3 * GIB} rows A:{fms['A'].n_far}x{c['r']} W:{fms['W'].n_far}x{c['m']} "
          "mapped " + " ".join(f"{t}@2^{S.bit_length() - 1}:{fms[t].rows_at(S)}" for t in "AW"
                               for S in fms[t].seams))
    p64 = {k: v.astype(np.float64) for k, v in p0.items()}
    rr = slice(0, RANK_ROWS)
    B, ref = _padding_bias(c, p64, xs.xFeats[rr], prob["a1"][rr], prob["a2"][rr],
                           fms["A"].n_far - RANK_N)
    print(f"PADBIAS {tag} B {B}")
    nq = 64
    Q = ref["q"][:nq, 0].astype(np.float32)
    add = ref["c"][:nq, 0].astype(np.float32)
    res = {}
    for name, f in (("compact", {"A": None, "W": None}), ("far", fms)):
        run = _FarRun(c, cuda_dev, f, None, pads={"A": 0.0, "Ab": -B}, problem=prob)
        try:
            rows = run.rows["A"]
            res[name] = _entries(run, c, rows[prob["a1"]], rows[prob["a2"]],
                                 rows[prob["neg1"]].astype(np.int32),
                                 rows[prob["neg2"]].astype(np.int32), Q, add, rows[prob["a1"][:nq]])
            if name == "far":
                viol = [f"{k}: {bad[:4]}" for k, t in TABLE_OF.items()
                        for bad in [F.padding_violations(run.named[k], run.pads[k], run.rows[t])]
                        if bad.size]
                assert not viol, viol
        finally:
            run.close()
    far, cmp_ = res["far"], res["compact"]
    mapA = fms["A"].rows
    through = lambda e: np.where(e >= 0, mapA[np.maximum(e, 0)], -1)
    diff = [k for k in ("terms", "sums", "target", "greater", "equal", "arg_scores", "argx_scores",
                        "q_scores", "psi", "rel_psi", "rel_joint", "rel_dec", "rel_joint_labels",
                        "labels", "probs") if far[k].tobytes() != cmp_[k].tobytes()]
    diff += [k for k in ("arg_ents", "argx_ents", "q_ents")
             if not np.array_equal(far[k], through(cmp_[k]))]
    if far["ranks"] != cmp_["ranks"]:
        diff.append("ranks")
    print(f"BITWISE {tag} {'equal' if not diff else 'DIFFERS: ' + ', '.join(diff)}")
    # against float64
    host = _Split(prob["a1"], prob["a2"], xs.xFeats)
    want, cost = _oracle(c["dec"], p64, host, slice(0, xs.xFeats.shape[0]), prob["neg1"],
                         prob["neg2"], alpha=c["alpha"])

    class _Res:
        terms = None
    import torch
    r_ = _Res()
    r_.terms, r_.cost = torch.as_tensor(far["terms"]), far["cost"]
    _check(r_, want, cost, tag)
    gr, eq = far["greater"], far["equal"]
    assert not ((gr < ref["lo"]) | (gr + eq > ref["hi"])).any()
    err = np.abs(far["lse"].astype(np.float64) - ref["lse"])
    print(f"LSE {tag} max |lse - lse64| {err.max():.3e}, smallest bound {ref['lse_bound'].min():.3e}")
    assert np.all(err <= ref["lse_bound"])
    assert not diff, diff


@pytest.mark.timeout(300)
def test_far_rows_label_probs_past_2e31(built_lib, cuda_dev):
    """rae_label at m = 512 with W far (d_far m >= 2^31) over ceil(2^31 / m) + 64 CSR rows, so
    that probs itself passes 2^31 elements: all rows are empty except 200 real ones placed by
    far_map.  The real rows equal the compact call bitwise; every empty row holds one and the
    same row, argmax(Wb) and softmax(Wb) (against float64 at test_gpu_eval's TERM tolerances)."""
    import torch
    from _entry_ref import csr_of_lengths
    from rae import _lib
    from test_gpu_eval import TERM_ATOL, TERM_RTOL
    m, d, nreal = 512, 400, 200
    g = np.random.RandomState(11)
    lens = g.randint(0, 13, size=nreal)
    lens[[0, 7]] = 0                            # empty rows among the real ones
    X = csr_of_lengths(g, lens, d)
    W = (g.standard_normal((d, m)) * 0.4).astype(np.float32)
    Wb = (g.standard_normal(m) * 0.5).astype(np.float32)
    cw = np.bincount(X.indices, minlength=d)[None, :]
    fw = F.far_map(cw, m)
    fr = F.far_map(np.ones((1, nreal), np.int64), m)        # the rows of labels / probs
    assert not F.check_map(fw, cw) and not F.check_map(fr, np.ones((1, nreal), np.int64))
    nrows = fr.n_far
    assert nrows * m > 2 ** 31 and fw.n_far * m > 2 ** 31
    need = 4 * m * (fw.n_far + nrows) + 8 * nrows + 2 * GIB
    _skip_unless_fits(need)
    tag = "label-m512-W+probsfar"
    print(f"FAR {tag} bytes {need - 2 * GIB} rows W:{fw.n_far}x{m} probs:{nrows}x{m} mapped " +
          " ".join(f"{t}@2^{S.bit_length() - 1}:{f.rows_at(S)}" for t, f in (("W", fw), ("probs", fr))
                   for S in f.seams))
    p, up = _lib.ptr, lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dtype=dt), device=cuda_dev)

    def label(indptr, indices, values, Wt, n):
        lab = torch.full((n,), -7, dtype=torch.int64, device=cuda_dev)
        pr = torch.full((n, m), float("nan"), dtype=torch.float32, device=cuda_dev)
        _lib.check(built_lib.rae_label(p(indptr), p(indices), p(values), p(Wt), p(Wbt), m, 0, n,
                                       p(lab), p(pr), None), "rae_label")
        torch.cuda.synchronize()
        return lab, pr
    Wbt = up(Wb, np.float32)
    Wf = lab_f = pr_f = empty = None
    try:
        lab_c, pr_c = label(up(X.indptr, np.int32), up(X.indices, np.int32), up(X.data, np.float32),
                            up(W, np.float32), nreal)
        lab_c, pr_c = lab_c.cpu().numpy(), pr_c.cpu().numpy()
        # the far problem: the real rows in far-row order, their features in the compact order
        order = np.argsort(fr.rows)
        lens_far = np.zeros(nrows, np.int64)
        lens_far[fr.rows] = lens
        indptr = np.concatenate([[0], np.cumsum(lens_far)])
        cols = np.concatenate([fw.rows[X.indices[X.indptr[i]:X.indptr[i + 1]]] for i in order])
        vals = np.concatenate([X.data[X.indptr[i]:X.indptr[i + 1]] for i in order])
        Wf = torch.full((fw.n_far, m), 0.125, dtype=torch.float32, device=cuda_dev)
        F.scatter_rows(Wf, fw.rows, W)
        lab_f, pr_f = label(up(indptr, np.int32), up(cols, np.int32), up(vals, np.float32), Wf, nrows)
        same = (np.array_equal(F.gather_rows(lab_f, fr.rows), lab_c) and
                F.gather_rows(pr_f, fr.rows).tobytes() == pr_c.tobytes())
        print(f"BITWISE {tag} {'equal' if same else 'DIFFERS'}")
        # the empty rows: one closed-form row
        empty = torch.as_tensor(pr_c[0], device=cuda_dev)
        S = Wb.astype(np.float64)
        want = np.exp(S - S.max()) / np.exp(S - S.max()).sum()
        np.testing.assert_allclose(pr_c[0].astype(np.float64), want, rtol=TERM_RTOL, atol=TERM_ATOL)
        assert lab_c[0] == int(np.argmax(S))
        live = fr.rows[lens > 0]
        off = F.padding_violations(pr_f, empty, live)
        offl = F.padding_violations(lab_f, int(lab_c[0]), live)
        print(f"PADDING {tag} {'clean' if not off.size + offl.size else (off[:4], offl[:4])}")
        assert same
        assert off.size == 0 and offl.size == 0, (off[:8], offl[:8])
        assert F.padding_violations(Wf, 0.125, fw.rows).size == 0
    finally:
        Wf = lab_f = pr_f = empty = None
        _free_device()
