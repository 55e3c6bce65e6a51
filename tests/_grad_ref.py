"""Host references for one training step under every optimiser / regulariser option
(tests/test_grad_ref.py pins them on the CPU; tests/test_gpu_options.py holds the device to them at
one rank, tests/test_gpu_dp_options.py the data-parallel forms at the same global batch).

* a dataset whose batches hold every row class of the update (rows of the A and of the W table
  with exactly 1 record, 2-4, 5-16 and more than 16 records), and a "hot" variant with a row
  of at least 256 records (the heavy-row chunks);
* generic parameters (no zero biases, no near-uniform P) in place of the reference
  initialisation;
* three references for the gradients of one step: the analytic float64 oracle
  (rae_oracle.train_step_grads), the same with the bf16 operand rounding emulated, and
  autograd of cpu_ref.cost_graph (float64: a second derivation; float32: the yardstick for
  what single precision costs at these parameters);
* the metric rho and the extraction of the gradient from the device's state after one step.
"""
import functools
import math
import sys

import numpy as np
import torch

import cpu_ref
import rae_oracle as O

ROW_CLASSES = ((1, 1), (2, 4), (5, 16), (17, 1 << 30))
FLOOR = 2.0 ** -20          # floor of the float32 yardstick
FACTOR = 16.0               # device <= FACTOR * max(host float32, FLOOR), both against float64
LAMBDA1, LAMBDA2 = 0.01, 0.1

# option sets: optimiser, lambda1, lambda2, ext_reg, alpha, non-binary feature values, lr
OPTIONS = {
    "O0": dict(opt="adagrad", l1=0.0, l2=0.0, ext_reg=True, alpha=1.0, values=False, lr=0.1),
    "O1": dict(opt="adagrad", l1=LAMBDA1, l2=LAMBDA2, ext_reg=True, alpha=0.1, values=True, lr=0.1),
    "O2": dict(opt="adagrad", l1=LAMBDA1, l2=LAMBDA2, ext_reg=False, alpha=1.0, values=False, lr=0.1),
    "O3": dict(opt="sgd", l1=0.0, l2=0.0, ext_reg=True, alpha=0.1, values=True, lr=1.0),
    "O4": dict(opt="sgd", l1=LAMBDA1, l2=LAMBDA2, ext_reg=True, alpha=1.0, values=False, lr=1.0),
}

# shapes: decoder, (m, r, s, l), d, bf16 operands, kernel forms asked for, forms expected
SHAPES = {
    "S1": dict(dec="sp", mrsl=(100, 200, 20, 100), d=3000, want={"sp_forward": "fused"}),
    "S2": dict(dec="sp", mrsl=(30, 100, 10, 60), d=500, want={"sp_forward": "fused"}),
    "S3": dict(dec="sp", mrsl=(7, 13, 3, 70), d=700, want={"sp_forward": "fused"}),
    "S4": dict(dec="sp", mrsl=(8, 44, 5, 37), d=500, forms={"sp_forward": "split"},
               want={"sp_forward": "split"}),
    "S5": dict(dec="sp", mrsl=(300, 300, 50, 37), d=1500, want={"sp_forward": "split"}),
    "B1": dict(dec="rescal", mrsl=(100, 200, 20, 100), d=2000),
    "B2": dict(dec="rescal", mrsl=(7, 13, 3, 70), d=700),
    "B3": dict(dec="rescal", mrsl=(400, 24, 3, 40), d=600),
    "B4": dict(dec="rescal", mrsl=(100, 200, 20, 100), d=2000, bf16=True),
    "B5": dict(dec="rescal", mrsl=(60, 96, 5, 40), d=800, bf16=True),
    "B6": dict(dec="rescal", mrsl=(132, 24, 3, 40), d=600, bf16=True),
    "H1": dict(dec="rescal+sp", mrsl=(30, 60, 10, 100), d=1000),
    "H2": dict(dec="rescal+sp", mrsl=(7, 13, 3, 70), d=700),
    "H3": dict(dec="rescal+sp", mrsl=(100, 200, 20, 100), d=2000, bf16=True),
    "X1": dict(dec="sp", mrsl=(8, 16, 4, 256), d=300, hot=True, forms={"heavy_chunk": "on"},
               want={"heavy_chunk": "on"}),
    "X2": dict(dec="rescal+sp", mrsl=(8, 16, 4, 256), d=300, hot=True,
               forms={"heavy_chunk": "on"}, want={"heavy_chunk": "on"}),
}

ALL_OPTIONS = ("S1", "S3", "B1", "B4", "H1")
CASES = [(sh, op) for sh in SHAPES
         for op in (tuple(OPTIONS) if sh in ALL_OPTIONS else ("O1", "O3"))]
N_BATCHES = 3

# Data-parallel cases (tests/test_gpu_dp_options.py).  A shape's batch is the GLOBAL batch L of
# G ranks with l = L / G examples each, so the references of a case are those of the single-rank
# case at l = L.  DP_SHAPES adds what SHAPES lacks: S4p, the forced split SP forward at L = 36
# (three ranks of 12).
DP_SHAPES = dict(SHAPES)
DP_SHAPES["S4p"] = dict(dec="sp", mrsl=(8, 44, 5, 36), d=500, forms={"sp_forward": "split"},
                        want={"sp_forward": "split"})


def _dp_cases():
    """(shape, option, G, dp_dense, priv_rows, partitioned): dp_dense / priv_rows None leave the
    form to the plan; partitioned cases run the replicated update too (same forms) and compare
    the two bitwise.  A regulariser (O1, O4) goes with the replicated update only."""
    out = []

    def add(shape, option, G, dense=None, priv=None, part=False):
        out.append((shape, option, G, dense, priv, part))
    for G in (2, 4):
        for dense in ("records", "partials"):
            for op in ("O1", "O3", "O4"):
                add("S1", op, G, dense)
    for dense in ("partials", "records"):
        for priv in ("on", "off"):
            for op in ("O0", "O3"):
                add("S1", op, 2, dense, priv, True)
    for G in (2, 5):                        # the scalar path; G = 5: 14 rows owned of L = 70
        for dense in ("records", "partials"):
            for op in ("O1", "O3"):
                add("S3", op, G, dense, None, G == 5 and op == "O3")
    for op in ("O1", "O3"):
        add("S4p", op, 3, "partials")
        add("B1", op, 2, part=op == "O3")
        add("B2", op, 2)
    for op in ("O1", "O3", "O4"):
        add("H1", op, 4, part=op == "O3")
    for op in ("O1", "O3"):
        add("B4", op, 2)
        add("B5", op, 2, part=op == "O3")   # L = 40: Lp = 64 has 24 padding examples
    add("B6", "O3", 2)                      # m > 128
    add("H3", "O3", 2)
    for shape in ("X1", "X2"):
        add(shape, "O3", 2, part=True)
        add(shape, "O1", 2)
    return out


DP_CASES = _dp_cases()


def dp_case_id(case):
    shape, option, G, dense, priv, part = case
    return (f"{shape}-{option}-G{G}" + (f"-{dense}" if dense else "") +
            (f"-priv_{priv}" if priv else "") + ("-part" if part else ""))


def dp_case_config(shape, option):
    """The global-batch config of a data-parallel case (l is the global batch L)."""
    return case_config(shape, option, DP_SHAPES)


def case_config(shape, option, shapes=None):
    """Everything one (shape, option) case needs, as a dict."""
    c = dict((shapes or SHAPES)[shape])
    c.update(OPTIONS[option])
    c["m"], c["r"], c["s"], c["l"] = c.pop("mrsl")
    c["n"] = 20000 if (c["l"], c["s"]) == (100, 20) else 4000
    c["N"] = N_BATCHES * c["l"]
    c.setdefault("bf16", False)
    c.setdefault("hot", False)
    c.setdefault("forms", {})
    c.setdefault("want", {})
    c["shape"], c["option"] = shape, option
    return c


# --------------------------------------------------------------------------------------------
# dataset
# --------------------------------------------------------------------------------------------
def _class_counts(counts):
    counts = counts[counts > 0]
    return [int(((counts >= lo) & (counts <= hi)).sum()) for lo, hi in ROW_CLASSES]


def batch_row_classes(data, neg1, neg2, l, b):
    """Rows of the A and of the W table per record-count class in batch b."""
    xs = data.split["train"]
    rows = slice(b * l, (b + 1) * l)
    ids = np.concatenate([xs.args1[rows], xs.args2[rows], neg1[:, rows].ravel(),
                          neg2[:, rows].ravel()])
    ca = np.bincount(ids, minlength=data.get_arg_voc_size())
    cw = np.bincount(xs.xFeats[rows].indices, minlength=data.get_dimensionality())
    return ca, cw


@functools.lru_cache(maxsize=None)
def options_dataset(l, s, n, d, hot=False, values=False):
    """(DatasetManager, neg1, neg2): features of synthetic_dataset(3 l, d, 6, seed=99), entities
    from a Zipf(1.2) vocabulary of n ids of its own, so a batch references most entity rows
    once, some a few times and a few very often -- synthetic_dataset's own n = N / 5 entities
    make every A row of a small batch very heavy.  Every batch holds every row class of both
    tables (asserted).  hot: the first four ids' frequencies are raised until every batch has
    a row of at least 256 records."""
    from rae.data import DatasetManager, DatasetSplit, synthetic_dataset
    N = N_BATCHES * l
    feats, _ = synthetic_dataset(N, d, 6, seed=99)
    X = feats.split["train"].xFeats.copy()
    if values:
        X.data = np.random.RandomState(5).uniform(0.5, 2.0, size=X.data.shape).astype(np.float32)
    base = np.ceil(n / np.power(1.0 + np.arange(n), 1.2)).astype(np.int64)
    boost = 1
    while True:
        freqs = base.copy()
        freqs[:4] *= boost
        g = np.random.RandomState(7)
        p = freqs / freqs.sum()
        a1 = g.choice(n, size=N, p=p).astype(np.int32)
        a2 = g.choice(n, size=N, p=p).astype(np.int32)
        a2[::7] = a1[::7]
        data = DatasetManager({"train": DatasetSplit(a1, a2, X)}, freqs, d)
        gn = np.random.RandomState(2)
        neg1 = O.negative_samples(gn, data.negSamplingCum, N, s)
        neg2 = O.negative_samples(gn, data.negSamplingCum, N, s)
        tops = [batch_row_classes(data, neg1, neg2, l, b)[0].max() for b in range(N_BATCHES)]
        if not hot or min(tops) >= 256:
            break
        boost *= 2
        assert boost <= 1 << 16
    for b in range(N_BATCHES):
        ca, cw = batch_row_classes(data, neg1, neg2, l, b)
        assert min(_class_counts(ca)) > 0, ("A row classes", l, s, b, _class_counts(ca))
        assert min(_class_counts(cw)) > 0, ("W row classes", l, s, b, _class_counts(cw))
        if hot:
            assert ca.max() >= 256, (b, ca.max())
    return data, neg1, neg2


def case_dataset(c):
    return options_dataset(c["l"], c["s"], c["n"], c["d"], c["hot"], c["values"])


# --------------------------------------------------------------------------------------------
# parameters
# --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _generic_params(decoder, d, m, n, r):
    g = np.random.RandomState(13)
    shapes = {"W": (d, m), "Wb": (m,), "A": (n, r), "Ab": (n,), "C1": (r, m), "C2": (r, m),
              "R": (r, r, m), "C": (r, r, m)}
    sd = {"W": 0.6, "A": 1.0 / math.sqrt(r)}
    p = {}
    for k in O.param_names(decoder):
        p[k] = g.normal(0.0, sd.get(k, 1.0), size=shapes[k]).astype(np.float32)
    return p


def generic_params(c):
    """fp32 parameters (as float32 arrays; do not modify): W ~ N(0, 0.6), A ~ N(0, r^-1/2),
    everything else N(0, 1), one RandomState(13) stream in parameter order."""
    return _generic_params(c["dec"], c["d"], c["m"], c["n"], c["r"])


def _p64(c):
    return {k: v.astype(np.float64) for k, v in generic_params(c).items()}


# --------------------------------------------------------------------------------------------
# references of one step
# --------------------------------------------------------------------------------------------
def _batch(c, b):
    data, neg1, neg2 = case_dataset(c)
    xs = data.split["train"]
    rows = slice(b * c["l"], (b + 1) * c["l"])
    return xs.xFeats[rows], xs.args1[rows], xs.args2[rows], neg1[:, rows], neg2[:, rows]


def oracle_step(c, b, bf16=False, params=None, **override):
    """rae_oracle.train_step_grads (float64) on batch b of the case: (cost, grads)."""
    X, e1, e2, n1, n2 = _batch(c, b)
    hp = dict(alpha=c["alpha"], lambda1=c["l1"], lambda2=c["l2"], adjust=c["l"] / c["N"],
              ext_reg=c["ext_reg"])
    hp.update(override)
    res = O.train_step_grads(c["dec"], _p64(c) if params is None else params,
                             X.astype(np.float64), e1, e2, n1, n2, bf16=bf16, **hp)
    return res.cost, res.grads


def autograd_step(c, b, dtype=torch.float64):
    """cpu_ref.cost_graph under torch autograd in `dtype`, plus the regulariser
    adjust (lambda1 sum|w| + lambda2 sum w^2) over rae_oracle.reg_names: (cost, grads)."""
    X, e1, e2, n1, n2 = _batch(c, b)
    names = O.param_names(c["dec"])
    p = {k: torch.tensor(v, dtype=dtype).requires_grad_(True) for k, v in generic_params(c).items()}
    Xt = cpu_ref.batch_csr(X, slice(None), dtype)
    ix = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64))
    cost = cpu_ref.cost_graph(c["dec"], p, Xt, ix(e1), ix(e2), ix(n1), ix(n2), c["alpha"])
    if c["l1"] != 0.0 or c["l2"] != 0.0:
        adjust = c["l"] / c["N"]
        for k in O.reg_names(c["dec"], c["ext_reg"]):
            cost = cost + adjust * (c["l1"] * p[k].abs().sum() + c["l2"] * p[k].square().sum())
    grads = torch.autograd.grad(cost, [p[k] for k in names])
    out = {}
    for k, gk in zip(names, grads):
        gk = gk.to_dense() if gk.is_sparse else gk
        out[k] = gk.detach().double().numpy()
    return float(cost.detach().double()), out


_REFS = {}


def references(c, b):
    """The references of batch b, computed once per (dataset, decoder, shape, option):
    dict(cost64, g64, cost32, g32, rho32 [, cost_emu, g_emu, rho_emu])."""
    key = (c["dec"], c["m"], c["r"], c["s"], c["l"], c["d"], c["hot"], c["option"], c["bf16"], b)
    if key not in _REFS:
        cost64, g64 = oracle_step(c, b)
        cost32, g32 = autograd_step(c, b, torch.float32)
        ref = dict(cost64=cost64, g64=g64, cost32=cost32, g32=g32,
                   rho32={k: rho(g32[k], g64[k]) for k in g64})
        if c["bf16"]:
            ref["cost_emu"], ref["g_emu"] = oracle_step(c, b, bf16=True)
            ref["rho_emu"] = {k: rho(ref["g_emu"][k], g64[k]) for k in g64}
        _REFS[key] = ref
    return _REFS[key]


# --------------------------------------------------------------------------------------------
# metric, tolerance, extraction
# --------------------------------------------------------------------------------------------
def _rows(x):
    x = np.asarray(x, dtype=np.float64)
    return x.reshape(1, -1) if x.ndim == 1 else x.reshape(-1, x.shape[-1])


def row_max(g):
    """max |g| of every row (rows along the last axis; a vector is one row), shaped to
    broadcast against g."""
    g = np.asarray(g, dtype=np.float64)
    if g.ndim == 1:
        return np.full(g.shape, np.abs(g).max(initial=0.0))
    return np.broadcast_to(np.abs(g).max(axis=-1, keepdims=True), g.shape)


def rho(x, g):
    """max |x - g| / rowmax |g| over the rows where g is not identically zero; where a row of
    g is exactly zero x must be exactly zero (inf otherwise)."""
    x2, g2 = _rows(x), _rows(g)
    rm = np.abs(g2).max(axis=1)
    zero = rm == 0.0
    if np.any(x2[zero] != 0.0):
        return math.inf
    if zero.all():
        return 0.0
    return float((np.abs(x2 - g2).max(axis=1)[~zero] / rm[~zero]).max())


def tolerance(rho32):
    """The fp32 tolerance on rho for a tensor whose float32 host gradient is rho32 from float64."""
    return FACTOR * max(rho32, FLOOR)


def extract_adagrad(p0, p1, acc, g_ref, tol):
    """The gradient a device AdaGrad step from a zero accumulator applied: |g| = sqrt(acc) (one
    fp32 rounding of g^2), the sign from p0 - p1 wherever |g_ref| > max(tol rowmax|g_ref|, 1e-11)
    (from 1e-11 up the step is at least 1e-6: more than an ulp of any |p| < 8); elsewhere only
    the magnitude is compared, i.e. the reference's sign is taken."""
    p0, p1, acc, g_ref = (np.asarray(v, dtype=np.float64) for v in (p0, p1, acc, g_ref))
    need = np.abs(g_ref) > np.maximum(tol * row_max(g_ref), 1e-11)
    sgn = np.where(need, np.sign(p0 - p1), np.where(g_ref < 0, -1.0, 1.0))
    return sgn * np.sqrt(acc)


def emulate_opt_update(p, acc, g, lr, opt):
    """csrc/rae_common.hpp opt_update in numpy float32: (p', acc')."""
    p, acc, g = (np.asarray(v, dtype=np.float32) for v in (p, acc, g))
    lr = np.float32(lr)
    if opt == "adagrad":
        a = (acc + g * g).astype(np.float32)
        step = ((lr * g).astype(np.float32) / (np.sqrt(a) + np.float32(1e-6))).astype(np.float32)
        return (p - step).astype(np.float32), a
    # SGD: one rounding of p - lr g (an fma)
    return (p.astype(np.float64) - np.float64(lr) * g.astype(np.float64)).astype(np.float32), acc


# --------------------------------------------------------------------------------------------
# the assertions of one step (tests/test_gpu_options.py, tests/test_gpu_dp_options.py; on the
# CPU tests/test_grad_ref.py feeds them planted states)
# --------------------------------------------------------------------------------------------
COST_RTOL = 2e-5            # tests/test_gpu_train.py
BF16_EXACT_FACTOR, BF16_EMU_FACTOR = 1.25, 0.25     # tests/test_gpu_fullscale.py
G = sys.modules[__name__]   # the names below are written as the tests write them


def _check_step(c, b, cost, p1, acc, tag, bad):
    """The assertions of one batch; failures are appended to `bad` (so every ratio of the case
    is printed before the test fails)."""
    ref = G.references(c, b)
    p0 = G.generic_params(c)
    lr = c["lr"]
    want = ref["cost64"]
    if c["bf16"]:
        dc = abs(ref["cost_emu"] - want)
        ok = (abs(cost - want) <= BF16_EXACT_FACTOR * dc + COST_RTOL * abs(want) and
              abs(cost - ref["cost_emu"]) <= BF16_EMU_FACTOR * dc + COST_RTOL * abs(want))
    else:
        ok = abs(cost - want) <= COST_RTOL * max(1.0, abs(want))
    print(f"COST {tag} b{b} gpu {cost:.9g} oracle {want:.9g} rel {abs(cost - want) / abs(want):.2e}")
    if not ok:
        bad.append(f"b{b} cost {cost!r} oracle {want!r}")
    for k, g64 in ref["g64"].items():
        t = G.tolerance(ref["rho32"][k])
        emu = ref["rho_emu"][k] if c["bf16"] else 0.0
        tol_exact = BF16_EXACT_FACTOR * emu + t
        a0 = p0[k].astype(np.float64)
        a1 = p1[k].astype(np.float64)
        rm = G.row_max(g64)
        # rows with an exactly zero gradient: never written
        zero = rm == 0.0
        if not np.array_equal(p1[k][zero], p0[k][zero]):
            bad.append(f"b{b} {k}: an untouched row changed")
        if c["opt"] == "adagrad":
            ak = acc[k].astype(np.float64)
            if np.any(ak[zero] != 0.0):
                bad.append(f"b{b} {k}: accumulator of an untouched row is not zero")
            g = G.extract_adagrad(a0, a1, ak, g64, tol_exact)
            # the step's size from the accumulator alone (its sign is in g, checked by rho)
            step = lr * np.sqrt(ak) / (np.sqrt(ak) + 1e-6)
            off = np.abs(np.abs(a0 - a1) - step)
            if not np.all(off <= 8 * 2.0 ** -24 * (np.abs(a0) + lr)):
                bad.append(f"b{b} {k}: p1 is not the AdaGrad step of sqrt(acc): {off.max():.3e}")
            slack = 0.0
        else:
            g = (a0 - a1) / lr
            slack = 2.0 ** -23 * np.abs(a1) / lr      # the one rounding of p1
        r_gpu = _rho_slack(g, g64, slack)
        ratio = r_gpu / max(ref["rho32"][k], G.FLOOR)
        line = (f"RATIO {tag} b{b} {k:2s} rho_gpu {r_gpu:.3e} rho_host32 {ref['rho32'][k]:.3e} "
                f"ratio {ratio:.3f}")
        if c["bf16"]:
            if c["opt"] == "adagrad":       # the sign rule against this reference's own tolerance
                g = G.extract_adagrad(a0, a1, ak, ref["g_emu"][k], BF16_EMU_FACTOR * emu + t)
            r_emu = _rho_slack(g, ref["g_emu"][k], slack)
            line += f" rho_emu {emu:.3e} rho_gpu_emu {r_emu:.3e}"
            if not r_emu <= BF16_EMU_FACTOR * emu + t:
                bad.append(f"b{b} {k}: rho(gpu, emu) {r_emu:.3e} > 0.25 * {emu:.3e} + {t:.3e}")
        print(line)
        if not r_gpu <= tol_exact:
            bad.append(f"b{b} {k}: rho(gpu, f64) {r_gpu:.3e} > {tol_exact:.3e} "
                       f"(host32 {ref['rho32'][k]:.3e}, ratio {ratio:.2f})")


def _rho_slack(x, g, slack):
    """rho(x, g) with a per-element allowance `slack` taken off |x - g| first (SGD: the rounding
    of p1, which is not the gradient's error)."""
    if np.isscalar(slack):
        return G.rho(x, g)
    err = np.maximum(np.abs(x - g) - slack, 0.0)
    zero = G.row_max(g) == 0.0
    if np.any(np.asarray(x)[zero] != 0.0):
        return float("inf")
    return G.rho(g + err, g)
