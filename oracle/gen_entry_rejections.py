"""Record what the plan-free evaluation entry points refuse, and the workspace sizes they ask for.

TEST INFRASTRUCTURE ONLY.  Builds the tree it stands in and writes
tests/golden/eval_entry_rejections.json: pure data (one argument change per line, the return
value and the exact rae_last_error() text), as tests/golden/plan_specs.json is for plan creation.
tests/test_entry_rejections.py replays the table against the built library, so a change to the
order, the wording or the reach of an argument check, or to a workspace layout, shows up as a
difference from the recorded behaviour.

Every case starts from well-formed arguments whose addresses are made up (suitably aligned, never
dereferenced: the method of tests/test_eval_host._args) and changes exactly one thing.  Every
recorded case must be refused with RAE_E_INVALID (a sizing function: -1), which happens before
the first HIP call; the generator asserts that and refuses to run where a GPU is visible.

Covered: rae_eval_cost / rae_eval_rank / rae_eval_topk / rae_eval_relations with the three
decoders, rae_rank_queries / rae_topk_queries / rae_relation_scores, and the four
*_workspace_bytes functions.

Usage:  python oracle/gen_entry_rejections.py [outfile]
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "eval_entry_rejections.json")

INVALID = -1                                   # RAE_E_INVALID
SP, RESCAL, HYBRID = 0, 1, 2
M0, R0 = 100, 200                              # multiples of 4: the 16-byte rules apply
N_ENT, NROWS, NQ, TOP = 1000, 1000, 100, 5

EVAL_ENTRIES = ("rae_eval_cost", "rae_eval_rank", "rae_eval_topk", "rae_eval_relations")
QUERY_ENTRIES = ("rae_rank_queries", "rae_topk_queries", "rae_relation_scores")
SIZERS = ("rae_eval_workspace_bytes", "rae_rank_workspace_bytes", "rae_topk_workspace_bytes",
          "rae_relscore_workspace_bytes")
SIZER_OF = {"rae_eval_cost": SIZERS[0], "rae_eval_rank": SIZERS[1], "rae_rank_queries": SIZERS[1],
            "rae_eval_topk": SIZERS[2], "rae_topk_queries": SIZERS[2],
            "rae_eval_relations": SIZERS[3], "rae_relation_scores": SIZERS[3]}


def _lib_mod():
    pkg = os.path.join(ROOT, "relation-autoencoder_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    from rae import _lib
    return _lib


def _fake(struct, fields):
    """Distinct made-up addresses, 64 KiB apart (so 256-byte aligned)."""
    for i, f in enumerate(fields):
        setattr(struct, f, 0x100000 + 0x10000 * i)


# ------------------------------------------------------------------ well-formed arguments
def eval_args(dec, m, r):
    a = _lib_mod().RaeEvalArgs()
    a.decoder, a.relations, a.embed, a.neg_samples = dec, m, r, 20
    a.n_entities, a.alpha = N_ENT, 1.0
    _fake(a, ("W", "Wb", "A", "Ab", "C1", "C2", "R3", "indptr", "indices", "args1", "args2",
              "neg1", "neg2", "sums_out", "workspace"))
    a.neg_stride, a.row0, a.nrows = NROWS, 0, NROWS
    return a


def rank_args(r):
    a = _lib_mod().RaeRankArgs()
    _fake(a, ("Q", "target", "A", "Ab", "greater", "equal", "workspace"))
    a.ldq, a.nq, a.n_entities, a.embed = r, NQ, N_ENT, r
    return a


def topk_args(r):
    a = _lib_mod().RaeTopkArgs()
    _fake(a, ("Q", "A", "Ab", "ents_out", "workspace"))
    a.ldq, a.nq, a.n_entities, a.embed, a.top = r, NQ, N_ENT, r, TOP
    return a


def relscore_args(dec, m, r):
    a = _lib_mod().RaeRelscoreArgs()
    a.decoder, a.relations, a.embed, a.n_entities = dec, m, r, N_ENT
    _fake(a, ("A", "C1", "C2", "R3", "e1", "e2", "psi_out"))
    a.nq, a.ldp, a.workspace, a.workspace_bytes = NQ, m, None, 0
    return a


def query_struct(fn, dec, m, r):
    """The caller-given-queries struct of an entry or sizing function (None: it has none)."""
    if fn in ("rae_rank_queries", "rae_rank_workspace_bytes"):
        return rank_args(r)
    if fn in ("rae_topk_queries", "rae_topk_workspace_bytes"):
        return topk_args(r)
    if fn in ("rae_relation_scores", "rae_relscore_workspace_bytes"):
        return relscore_args(dec, m, r)
    return None


def out_struct(entry):
    _lib = _lib_mod()
    if entry == "rae_eval_rank":
        o = _lib.RaeRankOut()
        _fake(o, ("greater", "equal"))
    elif entry == "rae_eval_topk":
        o = _lib.RaeTopkOut()
        _fake(o, ("ents",))
        o.top = TOP
    elif entry == "rae_eval_relations":
        o = _lib.RaeRelOut()
        _fake(o, ("psi", "joint", "labels_dec", "labels_joint"))
    else:
        return None
    return o


def _ref(s):
    return C.byref(s) if s is not None else None


def _size(lib, fn, q, e, top):
    if fn == "rae_eval_workspace_bytes":
        return int(lib.rae_eval_workspace_bytes(_ref(e)))
    if fn == "rae_topk_workspace_bytes":
        return int(lib.rae_topk_workspace_bytes(_ref(q), _ref(e), top))
    return int(getattr(lib, fn)(_ref(q), _ref(e)))


# ------------------------------------------------------------------ one case
def run(lib, case):
    """Build the case's well-formed arguments, apply its one change and make the call.
    Returns (return value, rae_last_error() text).

    case: {"fn", "decoder", "m", "r", "change": [op, target, field, value]} and, for a sizing
    function, "form": which structs are given ("q", "e", "both" or "neither").  op is "set"
    (field = value), "add" (field += value: a moved pointer, a count one short), "null" (the
    target struct is passed as NULL), "clear" (every field of the target struct is zero) or "none" (a sizing function's form alone is the case).
    target is "a" (the argument struct), "out" or "top" (a sizing function's parameter)."""
    fn, dec, m, r = case["fn"], case["decoder"], case["m"], case["r"]
    op, target, field, value = case["change"]
    q, e = query_struct(fn, dec, m, r), eval_args(dec, m, r)
    top = TOP
    if fn in SIZERS:
        form = case["form"]
        a = q if form == "q" else e
        out = None
    else:
        form = "e" if fn in EVAL_ENTRIES else "q"
        a = e if form == "e" else q
        out = out_struct(fn)
        if fn != "rae_relation_scores":        # its workspace is empty
            a.workspace_bytes = _size(lib, SIZER_OF[fn], q if form == "q" else None,
                                      e if form == "e" else None, top)
            assert a.workspace_bytes > 0, (case, lib.rae_last_error())
    if op in ("set", "add"):
        s = {"a": a, "out": out}.get(target)
        if target == "top":
            top = value
        elif op == "set":
            setattr(s, field, value)
        else:
            setattr(s, field, (getattr(s, field) or 0) + value)
    elif op == "clear":
        C.memset(C.byref(out), 0, C.sizeof(out))
    elif op == "null":
        if target == "a":
            a = None
        else:
            out = None
    if fn in SIZERS:
        if op == "null":                       # rae_eval_workspace_bytes(NULL)
            e = None
        rc = _size(lib, fn, q if form in ("q", "both") else None,
                   e if form in ("e", "both") else None, top)
    elif fn in ("rae_eval_cost",) + QUERY_ENTRIES:
        rc = int(getattr(lib, fn)(_ref(a), None))
    else:
        rc = int(getattr(lib, fn)(_ref(a), _ref(out), None))
    return rc, lib.rae_last_error().decode()


# ------------------------------------------------------------------ the cases
def _shape_changes(dec, rel=True, need_s=False):
    """One step outside each shape limit: (m, r, change) with the decoder held."""
    ch = [(M0, R0, ["set", "a", "decoder", 3]), (M0, R0, ["set", "a", "decoder", -1])] if rel else []
    if rel:
        ch += [(M0, R0, ["set", "a", "relations", v]) for v in (0, 513, 130)]
        if dec != SP:
            ch.append((M0, R0, ["set", "a", "relations", 324]))
    ch += [(M0, R0, ["set", "a", "embed", v]) for v in (0, 1025)]
    if need_s:
        ch.append((M0, R0, ["set", "a", "neg_samples", 0]))
    return ch


def _eval_entry_cases(fn, dec):
    ch = _shape_changes(dec, need_s=fn == "rae_eval_cost")
    if dec == HYBRID:                          # 16 (4 + 4 * 640) floats are more than 160 KiB
        ch.append((4, 636, ["set", "a", "embed", 640]))
    one = lambda *c: ch.append((M0, R0, list(c)))
    one("null", "a", "", None)
    for v in (0, 1 << 31):
        one("set", "a", "n_entities", v)
    one("set", "a", "nrows", -1)
    one("set", "a", "row0", -1)
    one("set", "a", "row0", (1 << 31) - NROWS)
    ptrs = ["W", "Wb", "A", "Ab"] + (["C1", "C2"] if dec != RESCAL else []) + \
        (["R3"] if dec != SP else []) + ["indptr", "indices", "args1", "args2", "workspace"]
    if fn == "rae_eval_cost":
        ptrs += ["neg1", "neg2", "sums_out"]
        one("add", "a", "neg_stride", -1)
    for p in ptrs:
        one("set", "a", p, None)
    for p in ("W", "Wb", "C1", "C2", "R3", "A"):
        one("add", "a", p, 4)
    one("add", "a", "workspace", 128)
    one("add", "a", "workspace_bytes", -1)
    if fn != "rae_eval_cost":
        one("null", "out", "", None)
    if fn == "rae_eval_rank":
        one("set", "out", "greater", None)
        one("set", "out", "equal", None)
    if fn == "rae_eval_relations":
        one("clear", "out", "", None)
    if fn == "rae_eval_topk":
        one("set", "out", "ents", None)
        one("set", "out", "top", 0)
        one("set", "out", "top", 33)
    return ch


def _query_entry_cases(fn, dec):
    rel = fn == "rae_relation_scores"
    ch = _shape_changes(dec, rel=rel)
    one = lambda *c: ch.append((M0, R0, list(c)))
    one("null", "a", "", None)
    for v in (0, 1 << 31):
        one("set", "a", "n_entities", v)
    one("set", "a", "nq", -1)
    if rel:
        one("add", "a", "ldp", -1)
        one("set", "a", "workspace_bytes", -1)
        one("set", "a", "workspace", 0x800080)
        ptrs = ["A"] + (["C1", "C2"] if dec != RESCAL else []) + (["R3"] if dec != SP else []) + \
            ["e1", "e2", "psi_out"]
        for p in ("C1", "C2", "R3"):
            one("add", "a", p, 4)
        for p in ("A", "psi_out", "e1", "e2"):  # the 4-byte rule: moved by 2
            one("add", "a", p, 2)
    else:
        one("add", "a", "ldq", -1)
        one("add", "a", "ldq", 2)
        ptrs = ["Q", "A", "workspace"] + \
            (["target", "greater", "equal"] if fn == "rae_rank_queries" else ["ents_out"])
        for p in ("Q", "A"):
            one("add", "a", p, 4)
        one("add", "a", "workspace", 128)
        one("add", "a", "workspace_bytes", -1)
        if fn == "rae_topk_queries":
            one("set", "a", "top", 0)
            one("set", "a", "top", 33)
    for p in ptrs:
        one("set", "a", p, None)
    return ch


def _sizer_cases(fn):
    """(form, decoder, m, r, change) of one sizing function."""
    only_e = fn == "rae_eval_workspace_bytes"
    out = []
    if only_e:
        out.append(("e", SP, M0, R0, ["null", "a", "", None]))
    else:
        out += [(f, SP, M0, R0, ["none", "", "", None]) for f in ("both", "neither")]
    for dec in (SP, RESCAL, HYBRID):
        ech = _shape_changes(dec, need_s=only_e)
        if dec == HYBRID:
            ech.append((4, 636, ["set", "a", "embed", 640]))
        if not only_e:                         # rae_eval_cost checks n_entities at the call
            ech += [(M0, R0, ["set", "a", "n_entities", v]) for v in (0, 1 << 31)]
        out += [("e", dec, m, r, c) for m, r, c in ech]
        rel = fn == "rae_relscore_workspace_bytes"
        if only_e or (dec != SP and not rel):  # the other query structs name no decoder
            continue
        qch = _shape_changes(dec, rel=rel)
        qch += [(M0, R0, ["set", "a", "n_entities", v]) for v in (0, 1 << 31)]
        out += [("q", dec, m, r, c) for m, r, c in qch]
    if fn == "rae_topk_workspace_bytes":
        out += [(f, SP, M0, R0, ["set", "top", "", v]) for f in ("q", "e") for v in (0, 33)]
    return out


def cases():
    out = []
    for fn in EVAL_ENTRIES + QUERY_ENTRIES:
        per_dec = fn in EVAL_ENTRIES or fn == "rae_relation_scores"
        gen = _eval_entry_cases if fn in EVAL_ENTRIES else _query_entry_cases
        for dec in (SP, RESCAL, HYBRID) if per_dec else (SP,):
            out += [dict(fn=fn, decoder=dec, m=m, r=r, change=c) for m, r, c in gen(fn, dec)]
    for fn in SIZERS:
        out += [dict(fn=fn, form=form, decoder=dec, m=m, r=r, change=c)
                for form, dec, m, r, c in _sizer_cases(fn)]
    return out


# ------------------------------------------------------------------ accepted shapes' sizes
SIZE_SHAPES = ((7, 13, None), (30, 60, None), (100, 200, None), (128, 200, None), (320, 24, None),
               (512, 1024, SP), (4, 636, HYBRID))      # (m, r, the one decoder or all three)
SIZE_ENTITIES = (1, 1000, (1 << 31) - 1)
SIZE_TOPS = (1, 32)


def size_case(lib, s):
    """The bytes a sizing function asks for: s = {"fn", "form", "decoder", "m", "r", "n", "top"}."""
    e = eval_args(s["decoder"], s["m"], s["r"])
    e.n_entities = s["n"]
    q = query_struct(s["fn"], s["decoder"], s["m"], s["r"])
    if q is not None:
        q.n_entities = s["n"]
    return _size(lib, s["fn"], q if s["form"] == "q" else None, e if s["form"] == "e" else None,
                 s["top"])


def size_specs():
    out = []
    for m, r, only in SIZE_SHAPES:
        for dec in (SP, RESCAL, HYBRID) if only is None else (only,):
            base = dict(decoder=dec, m=m, r=r)
            out.append(dict(fn=SIZERS[0], form="e", n=N_ENT, top=TOP, **base))
            for n in SIZE_ENTITIES:
                for form in ("e", "q"):
                    out.append(dict(fn=SIZERS[1], form=form, n=n, top=TOP, **base))
                    out.append(dict(fn=SIZERS[3], form=form, n=n, top=TOP, **base))
                    out += [dict(fn=SIZERS[2], form=form, n=n, top=t, **base) for t in SIZE_TOPS]
    return out


def record(outfile, cases, run, size_specs, size_case, size_ok):
    """Build the tree, make every call and write the table (gen_analysis_rejections.py shares it)."""
    sys.path.insert(0, ROOT)
    import torch
    assert not torch.cuda.is_available(), "made-up addresses: run this where no GPU is visible"
    import __graft_entry__ as ge
    ge.build()
    lib = _lib_mod().load()
    rej, sizes = [], []
    for c in cases:
        rc, msg = run(lib, c)
        assert rc == INVALID and msg, (c, rc, msg)
        rej.append(dict(c, rc=rc, msg=msg))
    for s in size_specs:
        b = size_case(lib, s)
        assert size_ok(s, b), (s, b)
        sizes.append(dict(s, bytes=b))
    with open(outfile, "w") as fh:             # one case per line
        fh.write('{"rejections": [\n')
        fh.write(",\n".join(json.dumps(c) for c in rej))
        fh.write('\n], "sizes": [\n')
        fh.write(",\n".join(json.dumps(s) for s in sizes))
        fh.write("\n]}\n")
    print(f"wrote {outfile}: {len(rej)} refused cases, {len(sizes)} sizes")


def main(outfile=OUT):
    record(outfile, cases(), run, size_specs(), size_case,
           lambda s, b: b >= 0 and (b > 0 or s["fn"] == SIZERS[3] and s["form"] == "q"))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
