"""The per-batch row index and the tables built from it (k_idx_count -> k_idx_scatter ->
k_idx_sort / k_idx_sort<big> -> k_build_tasks, k_build_dplists; csrc/rae_index.hpp, rae_dp.hpp)
against the numpy reference of tests/_index_ref.py, with == everywhere.

Every case builds a plan through TrainEngine with tiny parameters (m = r = 4), sets negatives the
test chose, builds the index of one to three batches, checks rae_check and reads every region back
(rae_index_read).  No step runs.  Entity and feature ids are constructed, not drawn, so the counts
land exactly on the seams each case is named for; tests/test_index_inputs.py checks on the CPU
that every case hits its edge and that the reference is consistent with itself."""
import math

import numpy as np
import pytest

import _index_ref as R

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------
# case construction
# ---------------------------------------------------------------------------------------------
def scatter(vals):
    """vals at positions scattered by a stride permutation (so the sorted order is not the
    input order)."""
    n = len(vals)
    step = next(p for p in (7919, 104729, 1299709, 15485863) if math.gcd(p, n) == 1) if n > 1 else 1
    out = np.empty(n, np.int64)
    out[(np.arange(n) * step) % n] = vals
    return out


def fill_ids(total, counts, single0):
    """total ids: id `i` c times for every (i, c) of counts, the rest distinct from single0 on."""
    used = sum(c for _, c in counts)
    vals = [np.full(c, i, np.int64) for i, c in counts] + [single0 + np.arange(total - used)]
    return scatter(np.concatenate(vals))


def feats_from(L, counts, pad=None, single0=5000):
    """Feature rows of L examples: feature f in c distinct examples for every (f, c); example b
    padded with features nobody else has up to pad[b]."""
    rows = [[] for _ in range(L)]
    o = 0
    for f, c in counts:
        assert c <= L
        for k in range(c):
            rows[(o + k) % L].append(f)
        o += 5
    nxt = single0
    for b, n in sorted((pad or {}).items()):
        while len(rows[b]) < n:
            rows[b].append(nxt)
            nxt += 1
    return [np.array(sorted(r), np.int64) for r in rows]


def one_feat(N, mod=50):
    return [np.array([b % mod], np.int64) for b in range(N)]


def mixed_ids(N, NJ, n):
    """Entity ids with repeats: e1 == e2 in every 5th example, negatives equal to the positives."""
    b, j = np.meshgrid(np.arange(N), np.arange(NJ), indexing="ij")
    ids = (5 * b + 11 * j + (b * j) % 13) % n
    ids[::5, 1] = ids[::5, 0]
    ids[1::4, 2] = ids[1::4, 0]
    ids[2::6, NJ - 1] = ids[2::6, 1]
    return ids.astype(np.int64)


def mixed_feats(N, d=1009):
    lens = [3, 0, 1, 300, 33, 32, 2, 17]
    return [np.array(sorted((17 * b + 7 * k) % d for k in range(lens[b % 8])), np.int64)
            for b in range(N)]


class Case:
    def __init__(self, name, l, s, ids, feats, *, G=1, rank=0, dec="sp", priv="auto", chunk="auto",
                 part=False, window=1, batches=(0, 1), n_ent=None, d=None, edge=None,
                 understate_nnz=None):
        self.name, self.l, self.s, self.G, self.rank, self.dec = name, l, s, G, rank, dec
        self.priv, self.chunk, self.part, self.window, self.batches = priv, chunk, part, window, batches
        self.ids, self.feats = np.asarray(ids, np.int64), feats
        self.N = len(feats)
        assert self.ids.shape == (self.N, 2 + 2 * s) and self.N % (l * G) == 0
        self.n_ent = n_ent or int(self.ids.max()) + 1
        self.d = d or max(int(f.max(initial=0)) for f in feats) + 1
        self.edge = edge
        self.understate_nnz = understate_nnz

    def inputs(self, ids=None):
        ids = self.ids if ids is None else ids
        s = self.s
        nf = np.array([len(f) for f in self.feats])
        return dict(indptr=np.concatenate([[0], np.cumsum(nf)]).astype(np.int64),
                    indices=np.concatenate(self.feats + [np.zeros(0, np.int64)]),
                    args1=ids[:, 0].copy(), args2=ids[:, 1].copy(),
                    neg1=np.ascontiguousarray(ids[:, 2:2 + s].T),
                    neg2=np.ascontiguousarray(ids[:, 2 + s:].T))

    def dims(self):
        inp = self.inputs()
        mbn, mrn = R.batch_nnz(inp["indptr"], self.l * self.G)
        if self.understate_nnz is not None:
            mbn = self.understate_nnz
        return R.plan_dims(l=self.l, s=self.s, G=self.G, rank=self.rank, part=self.part,
                           window=self.window, n_examples=self.N, max_batch_nnz=mbn,
                           max_row_nnz=mrn, priv_rows=self.priv, heavy_chunk=self.chunk)

    def refs(self, ids=None):
        dims, inp = self.dims(), self.inputs(ids)
        return dims, {g: R.build(inp, dims, g, self.dec, self.n_ent, self.d)
                      for g in range(self.batches[0], self.batches[0] + self.batches[1])}


def row_counts(T):
    return set(np.unique(T["kept_rows"], return_counts=True)[1].tolist())


def seg_counts(T, c):
    return [int(e - s) for sg in T["segs"] for _, s, e, _ in sg[c]]


# ---- slices and the record encoding ---------------------------------------------------------
POSBITS = {1: 30, 31: 26, 32: 26, 33: 25, 64: 25, 65: 24}


def slice_case(L):
    def edge(dims, refs):
        ref = refs[0]
        assert dims["posbits"] == POSBITS[L] and (L + R.IDX_EPS - 1) // R.IDX_EPS == {
            1: 1, 31: 1, 32: 1, 33: 2, 64: 2, 65: 3}[L]
        assert dims["priv"] == 1
        if L >= 31:
            nf = ref["desc"][:, 0]
            assert nf.max() == 300 > dims["dcap"] == 256 and nf.min() == 0
            assert (ref["ids"][:, 0] == ref["ids"][:, 1]).any()
            assert (ref["ids"][:, 2] == ref["ids"][:, 0]).any()
            # same row, distinct records, of one example
            sr = ref["A"]["srec"] // (2 + 2 * dims["s"])
            assert any((sr[s:e][1:] == sr[s:e][:-1]).any() for sg in ref["A"]["segs"]
                       for c in sg for _, s, e, _ in c)
            assert ref["pmask"].any()
    return Case(f"slice_L{L}", L, 2, mixed_ids(L, 6, 97), mixed_feats(L), edge=edge)


# ---- classes and the private seam -----------------------------------------------------------
def class_case(dec, priv):
    L, s = 48, 1
    cnts = [2, 4, 5, 16, 17]
    ids = fill_ids(L * 4, [(101 + i, c) for i, c in enumerate(cnts)], 1000).reshape(L, 4)
    pad = {0: 32, 1: 33}
    pad.update({b: 8 for b in range(2, 10)})
    feats = feats_from(L, [(201 + i, c) for i, c in enumerate(cnts)], pad)

    def edge(dims, refs):
        ref = refs[0]
        for T in (ref["A"], ref["W"]):
            assert {1, 2, 4, 5, 16, 17} <= row_counts(T)
            assert seg_counts(T, 0) == [5, 16] and seg_counts(T, 2) == [17]
            assert {2, 4} <= set(seg_counts(T, 1))
        nf = ref["desc"][:, 0]
        assert nf[0] == 32 and nf[1] == 33 and dims["priv"] == (priv == "on")
        NJ = 4
        light1 = [int(r) for sg in ref["A"]["segs"] for _, s_, e, r in sg[1] if e - s_ == 1]
        e2_light = [r for r in light1 if r % NJ == 1 and nf[r // NJ] <= 32]
        pm = ref["pmask"].view(np.uint32)
        if priv == "off":
            assert not pm.any() and len(ref["A"]["private_recs"]) == 0 and light1
        else:
            # the 33-feature example's one-record rows stay in the table; the 32-feature one's go
            assert pm[0, 0] and pm[0, 2] == (1 << 32) - 1 - sum(
                1 << p for p, f in enumerate(feats[0]) if f < 5000)
            assert not pm[1].any() and any(r // NJ == 1 for r in light1)
            # SP's e2 slot is never private, RESCAL's is
            assert bool(e2_light) == (dec == "sp")
            assert bool((pm[:, 0] >> 1 & 1).any()) == (dec != "sp")
    return Case(f"classes_{dec}_priv_{priv}", L, s, ids, feats, dec=dec, priv=priv, edge=edge)


def nj64_case():
    L, s = 4, 31
    ids = np.arange(L * 64).reshape(L, 64)

    def edge(dims, refs):
        pm = refs[0]["pmask"].view(np.uint32)
        assert dims["priv"] == 1 and (pm[:, 0] == 0xfffffffd).all() and (pm[:, 1] == 0xffffffff).all()
    return Case("nj64_priv", L, s, ids, one_feat(L, 1), priv="on", edge=edge)


# ---- partitions -------------------------------------------------------------------------------
def w_1024_1025_case():
    l, s = 64, 1
    feats = [np.array(sorted(k * 31 + b % 31 for k in range(16)), np.int64) for b in range(2 * l)]
    feats[2 * l - 1] = np.append(feats[2 * l - 1], 600)

    def edge(dims, refs):
        assert (refs[0]["W"]["nrec"], refs[0]["W"]["H"]) == (1024, 1)
        assert (refs[1]["W"]["nrec"], refs[1]["W"]["H"]) == (1025, 2)
        assert dims["RW"] == 1025 and dims["HW"] == 2
    return Case("w_1024_one_partition_1025_two", l, s, mixed_ids(2 * l, 4, 97), feats, window=2,
                batches=(0, 2), edge=edge)


def a_2048_case():
    l, s = 256, 3
    ids = 2 * ((np.arange(l * 8) * 5) % 700).reshape(l, 8)

    def edge(dims, refs):
        A = refs[0]["A"]
        assert A["H"] == 2 and A["count"].tolist() == [R.IDX_FAST, 0]
    return Case("a_2048_keys_register_sort_full_other_partition_empty", l, s, ids, one_feat(l), edge=edge)


def a_2049_case():
    l, s = 257, 3
    vals = np.concatenate([3 * (np.arange(2049) % 600), [1, 2, 4, 5, 7, 8, 10]])
    ids = scatter(vals).reshape(l, 8)

    def edge(dims, refs):
        A = refs[0]["A"]
        assert A["H"] == 3 and A["count"].tolist() == [R.IDX_FAST + 1, 4, 3]
    return Case("a_2049_keys_lds_sort", l, s, ids, one_feat(l), edge=edge)


def a_8192_case():
    l, s = 1024, 3
    vals = 8 * ((np.arange(8192) * 7) % 3001)
    vals[:40] = 8 * 5000                       # and one very heavy row inside the big sort
    ids = scatter(vals).reshape(l, 8)

    def edge(dims, refs):
        A = refs[0]["A"]
        assert A["H"] == 8 and A["count"].tolist() == [R.KCAP] + [0] * 7
    return Case("a_8192_keys_lds_sort_full", l, s, ids, one_feat(l), edge=edge)


# ---- the dispatch table -----------------------------------------------------------------------
def tasks_case():
    l, s = 128, 8
    ids = scatter(np.arange(l * 18)).reshape(l, 18)

    def edge(dims, refs):
        ref = refs[0]
        assert ref["A"]["H"] == 3 and dims["priv"] == 0
        assert ref["thdr"][0] > R.TASK_PER and ref["A"]["pcls"][:, 1].tolist() == [768] * 3
    return Case("tasks_second_range_three_partitions", l, s, ids, one_feat(l), priv="off", edge=edge)


def nvc_case():
    l, s = 64, 8
    ids = fill_ids(l * 18, [(100 + i, 17) for i in range(34)], 1000).reshape(l, 18)
    feats = feats_from(l, [(10 + i, 17) for i in range(6)], {b: 2 for b in range(l)})

    def edge(dims, refs):
        ref = refs[0]
        assert dims["NVC"] == 32 and ref["n_very"] == 40 and ref["thdr"][1] == 32
        over = ref["task"][ref["n_wave_rows"]:, 0]
        assert len(over) == 8 and (over >= 0).sum() == 2 and (over < 0).sum() == 6
    return Case("very_heavy_rows_beyond_nvc", l, s, ids, feats, priv="off", edge=edge)


def chunk_case():
    l, s = 384, 1
    cnts = [255, 256, 383, 384]
    ids = fill_ids(l * 4, [(300 + i, c) for i, c in enumerate(cnts)], 1000).reshape(l, 4)
    feats = feats_from(l, [(10 + i, c) for i, c in enumerate(cnts)])

    def edge(dims, refs):
        ref = refs[0]
        assert dims["hch"] == 128 and ref["thdr"][2] == 6
        assert ref["hfin"][:, 2].tolist() == [2, 2, 3, 2, 2, 3]
        un = ref["vtask"][ref["vtask"][:, 3] >= 0]
        assert (un[:, 2] - un[:, 1]).tolist() == [255, 255]
    return Case("chunks_255_256_383_384", l, s, ids, feats, priv="off", chunk="on", edge=edge)


# ---- the ring ---------------------------------------------------------------------------------
def ring_case():
    l, s, nb = 33, 2, 5
    ids = scatter(np.arange(l * nb * 6)).reshape(l * nb, 6)        # first negatives: all distinct

    def edge(dims, refs):
        assert dims["index_window"] == 3
        assert [g % 3 for g in refs] == [2, 0, 1]
    return Case("ring_wrap_and_rebuild", l, s, ids, mixed_feats(l * nb), window=3, batches=(2, 3),
                priv="off", edge=edge)


def ring_second_ids(case):
    """The second epoch's negatives: few ids, so every table is shorter than what the slots held."""
    ids = case.ids.copy()
    ids[:, 2:] = mixed_ids(case.N, 6, 11)[:, 2:]
    return ids


# ---- the partitioned update -------------------------------------------------------------------
def part_case(G, rank, l, s, tag=""):
    N = G * l

    def edge(dims, refs):
        ref = refs[0]
        assert dims["part"] == 1 and dims["priv"] == 0 and dims["dnx"] == l
        for T in (ref["A"], ref["W"]):
            assert (T["kept_rows"] % G == rank).all() and len(T["kept_rows"])
            assert T["H"] == R.index_partitions(-(-T["nrec"] // G))
        if tag == "HA4":
            assert G == 4 and dims["HA"] == 4 and ref["A"]["H"] == 1
        if tag == "H2":
            assert G == 4 and ref["A"]["H"] == 2 and (ref["A"]["count"] > 0).all()
        assert all(len(ref["dpl"][d, p, t]) for d in (0, 1) for p in range(G) if p != rank
                   for t in (0, 1))
    return Case(f"partitioned_G{G}_rank{rank}{'_' + tag if tag else ''}", l, s,
                mixed_ids(N, 2 + 2 * s, 997), mixed_feats(N), G=G, rank=rank, part=True,
                n_ent=997, d=1009, edge=edge)


HASH_N = 2 * 32 * R.DPL_KEYS + 4      # entities: a bit per owned row no longer fits the LDS


def hashpass_case():
    """Row lists by hash passes with a restart: each rank's 512 examples reference, among the
    rows the OTHER rank owns, two rows 8,000 times each and 2,432 more, all with row / G = 0 mod 3
    -- the first sizing (3 passes) puts all 18,432 occurrences into one pass of 16,384 keys; the
    restart with 6 passes separates the two rows (their row / G differ mod 6).  (More than 8,192
    occurrences of one row would overflow the row index's own partition.)"""
    G, l, s = 2, 512, 17
    NJ = 36
    i = np.arange(l * NJ - 16000)           # the others keep off the two rows' index partitions
    q = np.concatenate([np.full(8000, 300000), np.full(8000, 300003), 18 * (i // 4) + 3 * (i % 4)])
    ids = np.concatenate([scatter(q * 2 + 1).reshape(l, NJ),      # rank 0 reads odd rows (rank 1's)
                          scatter(q * 2).reshape(l, NJ)])         # rank 1 reads even rows (rank 0's)

    def edge(dims, refs):
        ref = refs[0]
        assert (HASH_N - 1 + G - 1) // G > 32 * R.DPL_KEYS
        assert ref["dp_passes"][0, 1, 0] == (3, 6) and ref["dp_passes"][1, 1, 0] == (3, 6)
        assert ref["dp_passes"][0, 1, 1] == (1, 1)
        assert len(ref["dpl"][0, 1, 0]) == len(ref["dpl"][1, 1, 0]) == 2434
        assert ref["A"]["H"] == 18 and ref["A"]["count"].max() <= R.KCAP
        # by pass, then ascending: not one ascending run
        assert (np.diff(ref["dpl"][0, 1, 0]) < 0).any()
    return Case("partitioned_hash_pass_restart", l, s, ids, one_feat(G * l), G=G, rank=0, part=True,
                n_ent=HASH_N, edge=edge)


# ---- the error paths --------------------------------------------------------------------------
def overflow_case(tab):
    l, s = 1025, 3
    vals = np.concatenate([9 * ((np.arange(8193) * 7) % 3001), [1, 2, 3, 4, 5, 6, 7]])
    if tab == "A":
        ids, feats = scatter(vals).reshape(l, 8), one_feat(l)
    else:
        ids = mixed_ids(l, 8, 997)
        flat = np.concatenate([9 * (np.arange(8193) % 3001), [1, 2, 3, 4, 5, 6, 7]])
        feats = [np.array(sorted(flat[b * 8:(b + 1) * 8]), np.int64) for b in range(l)]
        assert all(len(set(f)) == 8 for f in feats)

    def edge(dims, refs):
        T = refs[0][tab]
        assert T["H"] == 9 and T["count"].tolist() == [R.KCAP + 1] + [1] * 7 + [0]
        other = refs[0]["W" if tab == "A" else "A"]
        assert other["count"].max() <= R.KCAP
    return Case(f"partition_of_8193_keys_{tab}", l, s, ids, feats, priv="off", edge=edge)


def capacity_case():
    l, s = 16, 1
    feats = [np.array(sorted((3 * b + 5 * k) % 101 for k in range(6 if b < l else 9)), np.int64)
             for b in range(2 * l)]

    def edge(dims, refs):
        assert dims["RW"] == 96 and refs[0]["W"]["nrec"] == 96 and refs[1]["W"]["nrec"] == 144
        assert refs[1]["n_very"] == 0
    return Case("batch_beyond_record_capacity", l, s, mixed_ids(2 * l, 4, 53), feats, window=2,
                batches=(0, 2), priv="off", understate_nnz=96, edge=edge)


CASES = [slice_case(L) for L in (1, 31, 32, 33, 64, 65)] + \
        [class_case(dec, priv) for dec in ("sp", "rescal") for priv in ("on", "off")] + \
        [nj64_case(), w_1024_1025_case(), a_2048_case(), a_2049_case(), a_8192_case(),
         tasks_case(), nvc_case(), chunk_case(), ring_case(),
         part_case(2, 0, 40, 2), part_case(2, 1, 40, 2), part_case(3, 2, 20, 2),
         part_case(4, 1, 32, 15, "HA4"), part_case(4, 3, 64, 15, "H2"), hashpass_case()]
ERROR_CASES = [overflow_case("A"), overflow_case("W"), capacity_case()]
BY_NAME = {c.name: c for c in CASES + ERROR_CASES}


# ---------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------
class NoPeers:
    """The ranks' exchange with no peers (one GPU): nothing travels; the list maxima the engine
    asks to agree on are kept for the test."""

    def __init__(self, G, rank):
        self.world_size, self.rank, self.maxima = G, rank, []

    def __call__(self, buf):
        pass

    def rows(self, send, recv):
        pass

    def max_int(self, v):
        self.maxima.append(int(v))
        return int(v)

    def sync_rows(self, ts):
        pass

    def barrier(self):
        pass


def make_engine(case, dev, monkeypatch=None):
    import scipy.sparse as sp
    from rae import engine as E
    from rae.data import DatasetManager
    from rae.model import OieModelFunctions, make_optimizer
    inp = case.inputs()
    X = sp.csr_matrix((np.ones(len(inp["indices"]), np.float32), inp["indices"], inp["indptr"]),
                      shape=(case.N, case.d))
    data = DatasetManager.from_arrays(X, inp["args1"], inp["args2"], n_entities=case.n_ent)
    mf = OieModelFunctions(np.random.RandomState(1), 4, 4, case.s, case.l, case.dec, data, True,
                           1.0, device=dev)
    if case.understate_nnz is not None:
        real = E.batch_nnz_stats
        monkeypatch.setattr(E, "batch_nnz_stats",
                            lambda ip, L: (case.understate_nnz, real(ip, L)[1]))
    forms = {"priv_rows": case.priv, "heavy_chunk": case.chunk,
             "dp_update": "partitioned" if case.part else "replicated"}
    eng = E.TrainEngine(mf, make_optimizer("sgd", mf.params), data.split["train"],
                        learning_rate=0.1, device=dev, world_size=case.G, rank=case.rank,
                        exchange=NoPeers(case.G, case.rank) if case.G > 1 else None,
                        index_window=case.window, kernel_forms=forms, index_overlap=False)
    # the arrays the plan reads are the case's
    x = data.split["train"].xFeats
    assert np.array_equal(x.indptr, inp["indptr"]) and np.array_equal(x.indices, inp["indices"])
    return eng, inp


def reader(eng, g):
    cache = {}

    def read(region):
        if region not in cache:
            cache[region] = eng.index_region(g, region)
        return cache[region]
    return read


@pytest.mark.parametrize("name", [c.name for c in CASES if not c.name.startswith("ring")])
def test_index_equals_reference(cuda_dev, name):
    case = BY_NAME[name]
    dims, refs = case.refs()
    eng, inp = make_engine(case, cuda_dev)
    try:
        assert eng.index_dims() == dims
        eng.set_epoch_negatives(inp["neg1"], inp["neg2"])
        eng.build_index(*case.batches)
        eng.check()
        for g, ref in refs.items():
            assert R.compare(ref, dims, reader(eng, g)) == [], (name, g)
        if case.part:
            want = [max(len(v) for (d, p, t), v in ref["dpl"].items() if t == tab)
                    for ref in refs.values() for tab in (0, 1)]
            assert eng.exchange.maxima == want          # dpmax, as rae_dp_list_max reported it
            assert eng.index_region(0, "dpmax").tolist() == [0, 0]
    finally:
        eng.close()


def test_ring_slots_reused_after_a_wrap(cuda_dev):
    """index_window = 3, batches [2, 5): slots 2, 0, 1 (the zeroing of the partition counts
    wraps); then new negatives and the same batches again -- shorter tables in the same slots, the
    first build's segments lying stale behind them."""
    case = BY_NAME["ring_wrap_and_rebuild"]
    eng, inp = make_engine(case, cuda_dev)
    try:
        for ids in (None, ring_second_ids(case)):
            dims, refs = case.refs(ids)
            inp = case.inputs(ids)
            eng.set_epoch_negatives(inp["neg1"], inp["neg2"])
            eng.build_index(*case.batches)
            eng.check()
            for g, ref in refs.items():
                assert R.compare(ref, dims, reader(eng, g)) == [], g
    finally:
        eng.close()


def test_region_read_rejects_what_the_plan_lacks(cuda_dev):
    import ctypes as C
    from rae import _lib
    case = BY_NAME["slice_L33"]
    eng, inp = make_engine(case, cuda_dev)
    try:
        buf = (C.c_int32 * 4)()
        lib, reg = eng.lib, _lib.INDEX_REGIONS
        for region in ("hfin", "dpl", "dpc", "dpmax"):
            assert lib.rae_index_read(eng.plan, 0, reg[region], buf, 16) == -1, region
        assert lib.rae_index_read(eng.plan, 0, reg["thdr"], buf, 12) == -1      # wrong size
        assert lib.rae_index_read(eng.plan, 0, 99, buf, 16) == -1
        assert lib.rae_index_read(eng.plan, 0, reg["thdr"], buf, 16) == 0
        v = (C.c_int64 * 23)()
        assert lib.rae_index_dims(eng.plan, v, 22) == -1
    finally:
        eng.close()
    off = BY_NAME["classes_sp_priv_off"]
    eng, _ = make_engine(off, cuda_dev)
    try:
        buf = (C.c_int32 * (4 * off.l))()
        assert eng.lib.rae_index_read(eng.plan, 0, _lib.INDEX_REGIONS["pmask"], buf, 16 * off.l) == -1
    finally:
        eng.close()


# ---- the error paths: an index built on a fresh plan, no step ---------------------------------
@pytest.mark.parametrize("tab", ["A", "W"])
def test_partition_overflow_is_reported(cuda_dev, tab):
    """A partition of 8193 keys: rae_check returns RAE_E_OVERFLOW and names bit 1 (A) / 2 (W);
    the other table of the batch is built as usual."""
    from rae import _lib
    case = BY_NAME[f"partition_of_8193_keys_{tab}"]
    dims, refs = case.refs()
    eng, inp = make_engine(case, cuda_dev)
    try:
        eng.set_epoch_negatives(inp["neg1"], inp["neg2"])
        eng.build_index(0, 1)
        assert eng.lib.rae_check(eng.plan) == -3
        msg = eng.lib.rae_last_error().decode()
        what = "an entity-row index partition" if tab == "A" else "a feature-row index partition"
        assert what in msg and f"flags={1 if tab == 'A' else 2})" in msg, msg
        with pytest.raises(_lib.RaeError):
            eng.check()
        read, o = reader(eng, 0), "W" if tab == "A" else "A"
        T = refs[0][o]
        n = len(T["srec"])
        assert np.array_equal(read("count" + o)[:T["H"]], T["count"])
        assert np.array_equal(read("pcls" + o)[:T["H"]], T["pcls"])
        assert np.array_equal(read("srec" + o)[:n], T["srec"])
        for p in range(T["H"]):
            want = np.concatenate(T["segs"][p])
            assert np.array_equal(read("seg" + o)[T["base"][p]:T["base"][p] + len(want)], want)
        # the overflowed table: its counts stand, the partition itself contributes no row
        B = refs[0][tab]
        assert np.array_equal(read("count" + tab)[:B["H"]], B["count"])
        assert read("pcls" + tab)[0].tolist() == [0, 0, 0, 0]
    finally:
        eng.close()


def test_capacity_overflow_is_reported(cuda_dev, monkeypatch):
    """max_batch_nnz understates batch 1: the device reports bit 4 ("a batch exceeded the row
    index's record capacity", include/rae.h), batch 0 is whole, and batch 1 has its entity table
    and no feature-row task."""
    case = BY_NAME["batch_beyond_record_capacity"]
    dims, refs = case.refs()
    eng, inp = make_engine(case, cuda_dev, monkeypatch)
    try:
        assert eng.index_dims() == dims
        eng.set_epoch_negatives(inp["neg1"], inp["neg2"])
        eng.build_index(0, 2)
        assert eng.lib.rae_check(eng.plan) == -3
        msg = eng.lib.rae_last_error().decode()
        assert "record capacity" in msg and "flags=4)" in msg, msg
        assert R.compare(refs[0], dims, reader(eng, 0)) == []
        read, ref = reader(eng, 1), refs[1]
        A = ref["A"]
        assert np.array_equal(read("countA")[:A["H"]], A["count"])
        assert np.array_equal(read("srecA")[:len(A["srec"])], A["srec"])
        assert not read("countW").any()
        a_only = ref["task"][ref["task"][:, 0] >= 0]
        assert read("thdr").tolist() == [len(a_only), 0, 0, 0]
        assert np.array_equal(read("task")[:len(a_only)], a_only)
    finally:
        eng.close()
