"""A plain numpy reference of the per-batch row index and the tables built from it, written
from the layout comments of csrc/rae_index.hpp, csrc/rae_dp.hpp and DESIGN.md section 2 -- one
np.lexsort and a few np.unique calls, no sorting network and no scans.  Everything here is an exact
integer function of a batch's entity ids, negatives and CSR rows, so the GPU tests compare with ==.

    dims = plan_dims(...)                      what the plan resolves (csrc/rae_plan.hpp)
    ref  = build(inp, dims, batch, dec)        the expected tables of one global batch
    check_invariants(ref, dims)                the reference's own consistency
    compare(ref, dims, read)                   against a read-back: only what the counts cover
"""
import numpy as np

HEAVY, VHEAVY = 4, 16           # more records than this: heavy / very heavy
IDX_PART = 1024                 # records per hash partition
IDX_HMAX = 1024                 # partition table entries per slot and table
IDX_FAST = 2048                 # keys the register sort takes; above: the LDS sort
KCAP = 8192                     # keys of the largest partition
IDX_EPS = 32                    # examples per slice of the binning launches
TASK_PER = 2048                 # dispatch table entries per workgroup of the table build
HCH = 128                       # records per chunk of a chunked very heavy row
DPL_KEYS = 16384                # keys per pass of a row list
NVC_MIN, NVC_DIV, PRIV_MAXL, HCH_MINL = 32, 2, 4096, 2048


def index_partitions(nrec):
    return 1 if nrec <= IDX_PART else (nrec + IDX_PART - 1) // IDX_PART


def batch_nnz(indptr, L):
    """(largest nnz of a whole global batch, longest example row)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    nb = (len(indptr) - 1) // L
    per = [int(indptr[(g + 1) * L] - indptr[g * L]) for g in range(nb)]
    return max(per + [1]), max(int(np.diff(indptr).max(initial=1)), 1)


def plan_dims(*, l, s, G, rank, part, window, n_examples, max_batch_nnz, max_row_nnz,
              priv_rows="auto", heavy_chunk="auto"):
    """The index dimensions of a plan without a regulariser (rae_index_dims' names)."""
    L, NJ = l * G, 2 + 2 * s
    RA, RW = L * NJ, max(max_batch_nnz, 1)
    nb = n_examples // L
    win = window if window > 0 else (256 if part else 2048)
    bbits = 1
    while (1 << bbits) < L:
        bbits += 1
    Lo = (L + G - 1) // G if part else L
    NVC = min(max(Lo // NVC_DIV, NVC_MIN), RA // (VHEAVY + 1) + 1 + RW // (VHEAVY + 1) + 1)
    hch = HCH if heavy_chunk == "on" or (heavy_chunk == "auto" and L >= HCH_MINL) else 0
    HF = (RA + RW) // hch + 1 if hch else 0
    if hch:
        NVC = max(NVC, HF + 1)
    dcap = min(max(max_row_nnz, 1), 256)
    priv = int(NJ <= 64 and (priv_rows == "on" or
                             (priv_rows == "auto" and not part and L < PRIV_MAXL)))
    return dict(L=L, l=l, s=s, G=G, rank=rank, part=int(part), RA=RA, RW=RW,
                HA=index_partitions(RA), HW=index_partitions(RW),
                index_window=max(1, min(win, nb)), posbits=31 - bbits, TC=RA + RW, NVC=NVC,
                hch=hch, HF=HF, dcap=dcap, dstride=(2 + NJ + dcap + 31) & ~31,
                dnx=L if (priv and G > 1) else l, priv=priv,
                privnf=min(dcap, 32) if priv else 0, LA=l * NJ if part else 0,
                LW=RW if part else 0)


def batch_ids(inp, dims, g):
    """(L, NJ) entity ids of global batch g: column j = 0 e1, 1 e2, 2+t neg1[t], 2+s+t neg2[t]."""
    L, s = dims["L"], dims["s"]
    e = slice(g * L, (g + 1) * L)
    return np.concatenate([inp["args1"][e, None], inp["args2"][e, None],
                           inp["neg1"][:, e].T, inp["neg2"][:, e].T], axis=1).astype(np.int64)


def batch_feats(inp, dims, g):
    """(feature id, example, position) of every CSR entry of global batch g, and the row lengths."""
    L = dims["L"]
    ip = np.asarray(inp["indptr"], dtype=np.int64)[g * L:(g + 1) * L + 1]
    nf = np.diff(ip)
    b = np.repeat(np.arange(L), nf)
    pos = np.arange(ip[0], ip[-1]) - ip[b]
    return np.asarray(inp["indices"][ip[0]:ip[-1]], dtype=np.int64), b, pos, nf


def _table(rows, recs, nf_of_rec, priv_ok, dims):
    """One table of one batch: rows / recs of all its records (flat)."""
    G, rank, part = dims["G"], dims["rank"], dims["part"]
    nrec = len(rows)
    H = index_partitions((nrec + G - 1) // G if part else nrec)
    keep = rows % G == rank if part else np.ones(nrec, bool)
    rows, recs, nf_of_rec, priv_ok = rows[keep], recs[keep], nf_of_rec[keep], priv_ok[keep]
    pid = (rows // G if part else rows) % H
    o = np.lexsort((recs, rows, pid))                     # by partition, then (row, record)
    rows, recs, pid = rows[o], recs[o], pid[o]
    count = np.bincount(pid, minlength=H).astype(np.int64)
    base = np.concatenate([[0], np.cumsum(count)[:-1]])
    n = len(rows)
    head = np.ones(n, bool)
    head[1:] = rows[1:] != rows[:-1]
    st = np.flatnonzero(head)
    en = np.append(st[1:], n)
    cnt = en - st
    private = np.zeros(len(st), bool)
    if dims["priv"]:
        private = (cnt == 1) & priv_ok[o][st] & (nf_of_rec[o][st] <= dims["privnf"])
    cls = np.where(cnt > VHEAVY, 2, np.where(cnt > HEAVY, 0, 1))
    seg = np.stack([rows[st], st, en, recs[st]], axis=1) if len(st) else np.zeros((0, 4), np.int64)
    segs, pcls = [], np.zeros((H, 4), np.int64)
    for p in range(H):
        mine = (pid[st] == p) & ~private
        by = [seg[mine & (cls == c)] for c in (0, 1, 2)]      # ascending row inside a class
        segs.append(by)
        pcls[p] = [len(by[0]), len(by[1]), len(by[2]), base[p]]
    return dict(nrec=nrec, H=H, kept_rows=rows, srec=recs, count=count, base=base, pcls=pcls,
                segs=segs, private_recs=recs[st[private]], private_rows=rows[st[private]])


def _dp_lists(inp, dims, g, ids, n_entities, n_features, pipe=False):
    """Partitioned update: per direction (0 send: peer p reads, I own; 1 recv: I read, peer p
    owns), peer and table the distinct rows rank x's l examples reference and rank y owns, by hash
    pass, then ascending (one pass: ascending)."""
    G, rank, l, L = dims["G"], dims["rank"], dims["l"], dims["L"]
    ip = np.asarray(inp["indptr"], dtype=np.int64)
    out, passes = {}, {}
    for d in (0, 1):
        for p in range(G):
            x, y = (p, rank) if d == 0 else (rank, p)
            for tab in (0, 1):
                if p == rank and not (pipe and d == 0):
                    out[d, p, tab] = np.zeros(0, np.int64)
                    continue
                if tab == 0:
                    cand = ids[x * l:(x + 1) * l].ravel()
                else:
                    e0 = g * L + x * l
                    cand = np.asarray(inp["indices"][ip[e0]:ip[e0 + l]], dtype=np.int64)
                own = cand[cand % G == y]
                nq = ((n_features if tab else n_entities) - y + G - 1) // G
                H0 = Hp = 1
                if nq > 32 * DPL_KEYS:         # hash passes (row / G) % Hp, each within DPL_KEYS
                    H0 = Hp = max(1, (2 * len(own) + DPL_KEYS - 1) // DPL_KEYS)
                    while np.bincount((own // G) % Hp, minlength=Hp).max(initial=0) > DPL_KEYS:
                        Hp *= 2
                u = np.unique(own)
                out[d, p, tab] = u[np.argsort((u // G) % Hp, kind="stable")]
                passes[d, p, tab] = (H0, Hp)             # first sizing, final
    return out, passes


def build(inp, dims, g, dec, n_entities=None, n_features=None):
    """Expected tables of global batch g.  dec: "sp" | "rescal" | "rescal+sp"."""
    L, NJ, s = dims["L"], 2 + 2 * dims["s"], dims["s"]
    ids = batch_ids(inp, dims, g)
    frow, fb, fpos, nf = batch_feats(inp, dims, g)
    j = np.tile(np.arange(NJ), L)
    b = np.repeat(np.arange(L), NJ)
    A = _table(ids.ravel(), b * NJ + j, nf[b], (j != 1) | (dec != "sp"), dims)
    W = _table(frow, (fb << dims["posbits"]) | fpos, nf[fb], np.ones(len(frow), bool), dims)
    ref = dict(A=A, W=W, ids=ids)
    # private rows: the example's mask words 0-1 hold the entity-slot bits j, word 2 the
    # feature-position bits
    pm = np.zeros((L, 4), np.uint32)
    if dims["priv"]:
        r = A["private_recs"]
        np.bitwise_or.at(pm, (r // NJ, (r % NJ) >> 5), np.uint32(1) << ((r % NJ) & 31).astype(np.uint32))
        r = W["private_recs"]
        pos = r & ((1 << dims["posbits"]) - 1)
        np.bitwise_or.at(pm, (r >> dims["posbits"], 2), np.uint32(1) << pos.astype(np.uint32))
    ref["pmask"] = pm.view(np.int32)

    def cls_list(T, c, w):
        parts = [sg[c] for sg in T["segs"]]
        out = np.concatenate(parts) if parts else np.zeros((0, 4), np.int64)
        out = out.copy()
        if w:
            out[:, 0] = ~out[:, 0]
        return out
    wave = np.concatenate([cls_list(A, 0, 0), cls_list(W, 0, 1), cls_list(A, 1, 0), cls_list(W, 1, 1)])
    very = np.concatenate([cls_list(A, 2, 0), cls_list(W, 2, 1)])
    hch, NVC = dims["hch"], dims["NVC"]
    nrecs = very[:, 2] - very[:, 1]
    chunked = (nrecs >= 2 * hch) if hch else np.zeros(len(very), bool)
    vt, hf = [], []
    for row, st, en, _ in very[chunked]:
        nch = (en - st) // hch
        hf.append((row, len(vt), nch, 0))
        for k in range(nch):
            c = len(vt)
            vt.append((row, st + k * hch, en if k + 1 == nch else st + (k + 1) * hch, -1 - c))
    un = very[~chunked]
    room = max(0, NVC - len(vt))
    vtask = np.array(vt + [tuple(x) for x in un[:room]], dtype=np.int64).reshape(-1, 4)
    task = np.concatenate([wave, un[room:]])
    ref["task"], ref["vtask"] = task, vtask
    ref["hfin"] = np.array(hf, dtype=np.int64).reshape(-1, 4)
    ref["thdr"] = np.array([len(task), len(vtask), len(hf), 0], dtype=np.int64)
    ref["n_wave_rows"], ref["n_very"], ref["n_overflow"] = len(wave), len(very), len(un[room:])
    # descriptors of the dnx examples: [nf, CSR start, NJ ids, first dcap feature ids, zeros]
    dnx, DS, dcap = dims["dnx"], dims["dstride"], dims["dcap"]
    first = 0 if dnx == L else dims["rank"] * dims["l"]
    ip = np.asarray(inp["indptr"], dtype=np.int64)
    desc = np.zeros((dnx, DS), np.int64)
    for bl in range(dnx):
        ex = g * L + first + bl
        k = min(int(ip[ex + 1] - ip[ex]), dcap)
        desc[bl, 0], desc[bl, 1] = ip[ex + 1] - ip[ex], ip[ex]
        desc[bl, 2:2 + NJ] = ids[first + bl]
        desc[bl, 2 + NJ:2 + NJ + k] = inp["indices"][ip[ex]:ip[ex] + k]
    ref["desc"] = desc
    if dims["part"]:
        ref["dpl"], ref["dp_passes"] = _dp_lists(inp, dims, g, ids, n_entities, n_features)
    return ref


def check_invariants(ref, dims, kcap=KCAP):
    """The reference against itself: every kept record once, in one segment's range or as one mask
    bit; the segment rows are the kept rows minus the private ones; the wave tasks, workgroup
    tasks and chunk ranges tile every non-private row exactly once."""
    NJ, pb = 2 + 2 * dims["s"], dims["posbits"]
    covered = {0: {}, 1: {}}
    entries = [tuple(int(v) for v in e) for e in ref["task"]]
    chunks = {}
    for e in ref["vtask"]:
        e = tuple(int(v) for v in e)
        if e[3] < 0:
            chunks.setdefault(e[0], []).append(e)
        else:
            entries.append(e)
    for row, c0, nch, _ in ref["hfin"]:
        cs = chunks.pop(int(row))
        assert [-1 - c[3] for c in cs] == list(range(c0, c0 + nch))
        assert all(cs[k][2] == cs[k + 1][1] for k in range(nch - 1))
        assert all(dims["hch"] <= c[2] - c[1] < 2 * dims["hch"] for c in cs)
        entries.append((int(row), cs[0][1], cs[-1][2], 0))
    assert not chunks
    for row, st, en, _ in entries:
        tab = 1 if row < 0 else 0
        row = ~row if row < 0 else row
        assert row not in covered[tab], (tab, row)
        covered[tab][row] = (st, en)
    for tab, T in ((0, ref["A"]), (1, ref["W"])):
        assert T["count"].sum() == len(T["srec"]) and T["H"] <= IDX_HMAX
        assert T["count"].max(initial=0) <= kcap
        all_segs = np.concatenate([np.concatenate(sg) for sg in T["segs"]])
        assert sorted(all_segs[:, 0]) == sorted(set(T["kept_rows"]) - set(T["private_rows"]))
        assert {int(r): (int(a), int(b)) for r, a, b, _ in all_segs} == covered[tab]
        in_segs = np.concatenate([T["srec"][a:b] for _, a, b, _ in all_segs] + [np.zeros(0, np.int64)])
        pm = ref["pmask"].view(np.uint32)
        bits = []
        for b, words in enumerate(pm):
            if tab == 0:
                bits += [b * NJ + j for j in range(NJ) if words[j >> 5] >> (j & 31) & 1]
            else:
                bits += [(b << pb) | p for p in range(32) if words[2] >> p & 1]
        assert sorted(bits) == sorted(T["private_recs"])
        assert sorted(np.concatenate([in_segs, np.array(bits, np.int64)])) == sorted(T["srec"])
        for p in range(T["H"]):                      # (row, record) order inside every row
            a, e = T["base"][p], T["base"][p] + T["count"][p]
            key = (T["kept_rows"][a:e] << 32) | T["srec"][a:e]
            assert np.all(np.diff(key) > 0)
    assert (pm[:, 3] == 0).all()
    assert ref["thdr"][1] <= dims["NVC"] and ref["thdr"][0] <= dims["TC"]
    assert ref["thdr"][2] <= max(dims["HF"], 0)


def compare(ref, dims, read):
    """ref against a read-back (read(region) -> int32 array): only what the counts cover -- per
    partition the first heavy + light + very heavy segments at its offset, task[:thdr[0]],
    vtask[:thdr[1]], hfin[:thdr[2]], lists up to their count.  Everything behind is stale by
    design and is not read.  Returns the list of differing tables (empty: all equal)."""
    bad = []

    def eq(name, got, want):
        got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
        if got.shape != want.shape or not np.array_equal(got, want):
            where = ""
            if got.shape == want.shape:
                i = np.argwhere(got != want)[0]
                where = f" first at {tuple(i)}: got {got[tuple(i)]}, want {want[tuple(i)]}"
            bad.append(f"{name}: shapes {got.shape} / {want.shape}{where}")
    for t, T in (("A", ref["A"]), ("W", ref["W"])):
        H, n = T["H"], len(T["srec"])
        eq("count" + t, read("count" + t)[:H], T["count"])
        eq("pcls" + t, read("pcls" + t)[:H], T["pcls"])
        eq("srec" + t, read("srec" + t)[:n], T["srec"])
        seg = read("seg" + t)
        for p in range(H):
            want = np.concatenate(T["segs"][p])
            eq(f"seg{t}[partition {p}]", seg[T["base"][p]:T["base"][p] + len(want)], want)
    thdr = read("thdr")
    eq("thdr", thdr, ref["thdr"])
    eq("task", read("task")[:ref["thdr"][0]], ref["task"])
    eq("vtask", read("vtask")[:ref["thdr"][1]], ref["vtask"])
    if dims["hch"]:
        eq("hfin", read("hfin")[:ref["thdr"][2]], ref["hfin"])
    eq("desc", read("desc"), ref["desc"])
    if dims["priv"]:
        eq("pmask", read("pmask"), ref["pmask"])
    if dims["part"]:
        dpl, dpc = read("dpl"), read("dpc")
        for (d, p, tab), want in ref["dpl"].items():
            eq(f"dpc[{d}][{p}][{tab}]", dpc[d, p, tab], len(want))
            off = dims["LA"] if tab else 0
            eq(f"dpl[{d}][{p}][{tab}]", dpl[d, p, off:off + len(want)], want)
    return bad
