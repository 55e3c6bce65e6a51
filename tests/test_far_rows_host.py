"""tests/_far_rows.py on the CPU: the far maps of every case tests/test_gpu_far_rows.py runs are
injective, in range, not monotone, use the rows that straddle the seams and give every record
class a row past every seam; and -- from the reference alone -- a kernel that evaluated a row
offset in int32, in uint32, or kept the byte offset modulo 2^32 would read, for every mapped row
such a fault moves, a location outside the table or contents that differ from the right row: none
of the three faults could reproduce the compact result.  The gather and padding helpers are
pinned on small tensors."""
import numpy as np
import pytest
import torch

import _far_rows as F
import _grad_ref as G

# (shape, option, table, top): the cases of tests/test_gpu_far_rows.py
A_CASES = [("S1", "O3"), ("S2", "O0"), ("S3", "O3"), ("S4", "O0"), ("S5", "O0"), ("U2", "O0"),
           ("B1", "O0"), ("B2", "O3"), ("B4", "O0"), ("H1", "O0"), ("X1", "O0"), ("X1", "O3")]
W_CASES = [("S1", "O1"), ("S3", "O3"), ("S5", "O0"), ("B4", "O0")]
MAP_CASES = ([(s, o, "A", 2 ** 31) for s, o in A_CASES] + [(s, o, "W", 2 ** 31) for s, o in W_CASES] +
             [("S1", "O0", "A", 2 ** 31), ("S1", "O0", "W", 2 ** 31), ("S3", "O3", "A", 2 ** 32)])


def case_counts(c):
    """(batches, n) records of every A row and (batches, d) of every W row."""
    data, neg1, neg2 = G.case_dataset(c)
    cc = [G.batch_row_classes(data, neg1, neg2, c["l"], b) for b in range(G.N_BATCHES)]
    return np.stack([x[0] for x in cc]), np.stack([x[1] for x in cc])


def case_map(c, table, top=2 ** 31):
    ca, cw = case_counts(c)
    counts, width = (ca, c["r"]) if table == "A" else (cw, c["m"])
    return F.far_map(counts, width, top), counts


def test_widths_are_the_issue_s():
    got_r = {G.case_config(s, o)["r"] for s, o, t, _ in MAP_CASES if t == "A"}
    got_m = {G.case_config(s, o)["m"] for s, o, t, _ in MAP_CASES if t == "W"}
    assert got_r == {200, 100, 13, 44, 300, 125, 60, 16} and got_m == {100, 7, 300}


@pytest.mark.parametrize("case", MAP_CASES, ids=["-".join(map(str, x)) for x in MAP_CASES])
def test_map_properties_and_teeth(case):
    shape, option, table, top = case
    c = G.case_config(shape, option)
    fm, counts = case_map(c, table, top)
    assert not F.check_map(fm, counts), F.check_map(fm, counts)
    w = fm.width
    assert fm.n_far * w > top and (fm.n_far - F.TAIL - 1) * w <= top
    for S in fm.seams:                  # the straddling row is used
        if S % w:
            k = fm.seam_rows[S]
            assert k * w < S < (k + 1) * w and k in set(fm.rows.tolist())
    if c["hot"] and table == "A":       # the >= 256-record row of every batch past 2^31 elements
        for b in range(G.N_BATCHES):
            hot = np.nonzero(counts[b] >= F.HOT)[0]
            assert hot.size and np.any(fm.rows[hot] * w >= 2 ** 31), b
    # teeth
    P = G.generic_params(c)[table]
    pad = 0.0 if (table == "W" and (c["l1"] or c["l2"])) else 0.25
    for fault in F.FAULTS:
        for whole in (False, True):
            hit, inside, same = F.wrapped_reads(fm, P, pad, fault, whole)
            first = {"int32": 2 ** 31, "uint32": 2 ** 32, "byte32": 2 ** 30}[fault]
            moved_rows = np.nonzero((fm.rows + 1) * w > first)[0]
            if whole:
                assert np.array_equal(hit, moved_rows), fault
            else:
                assert np.array_equal(hit, np.nonzero(fm.rows * w >= first)[0]), fault
            if first <= top:
                assert hit.size >= F.TAIL, (fault, hit.size)
            assert not same.any(), (fault, whole, fm.rows[hit[same]])
            if fault == "int32" and top == 2 ** 31:
                assert not inside.any()         # negative offsets: outside the table
            if fault == "byte32":
                assert inside.all()


def test_wrapped_location_on_another_mapped_row_is_seen():
    """A wrapped location that lands on a mapped row is compared by contents: two rows with equal
    contents, one 2^30 elements behind the other, hide the byte-offset fault, and wrapped_reads
    says so."""
    w = 16
    rows = np.array([3, 2 ** 30 // w + 3, 5, 2 ** 30 // w + 6])
    fm = F.FarMap(rows, 2 ** 31 // w + F.TAIL, w, 2 ** 31)
    g = np.random.RandomState(0)
    T = g.normal(size=(4, w)).astype(np.float32)
    hit, inside, same = F.wrapped_reads(fm, T, 0.25, "byte32", True)
    assert hit.tolist() == [1, 3] and inside.all() and not same.any()
    T[1] = T[0]                         # row 1 wraps onto row 0, which now holds the same values
    hit, inside, same = F.wrapped_reads(fm, T, 0.25, "byte32", True)
    assert same.tolist() == [True, False]
    T[3] = 0.25                         # row 3 wraps onto a padding row and equals the padding
    assert F.wrapped_reads(fm, T, 0.25, "byte32", False)[2].tolist() == [True, True]


def test_check_map_rejects_planted_maps():
    c = G.case_config("S3", "O3")
    fm, counts = case_map(c, "A")
    assert not F.check_map(fm, counts)
    mono = F.FarMap(np.sort(fm.rows), fm.n_far, fm.width, fm.top)
    assert any("monotone" in b for b in F.check_map(mono, counts))
    dup = F.FarMap(fm.rows.copy(), fm.n_far, fm.width, fm.top)
    dup.rows[1] = dup.rows[0]
    assert any("injective" in b for b in F.check_map(dup, counts))
    low = F.FarMap(np.random.RandomState(1).permutation(fm.rows.size), fm.n_far, fm.width, fm.top)
    bad = F.check_map(low, counts)
    assert any("has no row" in b for b in bad) and any("not all used" in b for b in bad)


def test_gather_scatter_and_padding_helpers():
    g = np.random.RandomState(3)
    t = torch.full((50, 7), 0.25)
    rows = np.array([41, 3, 17, 0, 49])
    vals = g.normal(size=(5, 7)).astype(np.float32)
    F.scatter_rows(t, rows, vals)
    assert np.array_equal(F.gather_rows(t, rows), vals)
    assert np.array_equal(F.gather_rows(t, [1, 2]), np.full((2, 7), 0.25, np.float32))
    # chunks of 3 rows (21 bytes of temporaries at a time), the last one short
    assert np.array_equal(F.rows_differing(t, 0.25, chunk_bytes=21), np.sort(rows))
    assert np.array_equal(F.rows_differing(t, 0.25), np.sort(rows))
    assert F.padding_violations(t, 0.25, rows).size == 0
    t[30, 6] = 0.25000003               # one element of one padding row, by one ulp
    assert F.padding_violations(t, 0.25, rows).tolist() == [30]
    t[31, 0] = float("nan")
    assert F.padding_violations(t, 0.25, rows).tolist() == [30, 31]
    v = torch.zeros(20)                 # a vector: rows of one element
    F.scatter_rows(v, np.array([19, 4]), np.array([1.0, -2.0], np.float32))
    assert F.rows_differing(v, 0.0, chunk_bytes=3).tolist() == [4, 19]
    assert F.gather_rows(v, [4, 19]).tolist() == [-2.0, 1.0]
    F.scatter_rows(v, np.array([4]), 0.0)
    assert F.rows_differing(v, 0.0).tolist() == [19]


def test_far_model_has_what_the_engine_reads():
    c = G.case_config("H1", "O0")
    p0 = G.generic_params(c)
    fm, _ = case_map(c, "A")
    rows = fm.rows[:50]                 # a small table on the CPU: 50 ids onto 64 rows
    small = np.argsort(np.argsort(rows))[::-1].copy()
    p = {k: (v[:50] if k in ("A", "Ab") else v) for k, v in p0.items()}
    named, acc = F.far_tensors(p, {"A": small, "Ab": small}, {"A": 64, "Ab": 64},
                               {"A": 0.25, "Ab": 0.25}, "cpu", True)
    model = F.FarModel(c["dec"], c["m"], c["r"], c["s"], c["l"], 64, c["alpha"], c["ext_reg"], named)
    assert model.param_names == ["W", "Wb", "C", "A", "Ab", "C1", "C2"]
    assert model.decoder.model_type == "rescal+sp" and model.n == 64
    assert [t.data_ptr() for t in model.params] == [named[k].data_ptr() for k in model.param_names]
    assert np.array_equal(F.gather_rows(named["A"], small), p["A"])
    assert F.padding_violations(named["A"], 0.25, small).size == 0
    assert F.padding_violations(named["Ab"], 0.25, small).size == 0
    assert all(float(a.abs().sum()) == 0.0 for a in acc.values())
    opt = F.FarOptimizer("adagrad", [acc[k] for k in model.param_names])
    assert opt.name == "adagrad" and len(opt.accumulator) == 7
