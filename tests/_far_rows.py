"""Relabelling invariance with inert padding: helpers of tests/test_far_rows_host.py (CPU) and
tests/test_gpu_far_rows.py (needs an MI355X).

A small case the suite already checks against float64 (tests/_grad_ref.py) has its entity (or
feature) ids mapped injectively onto rows of a table that ends just past 2^31 (or 2^32)
elements; every other row holds a padding value that cannot influence the result.  Only the rows
a batch touches are ever computed on, so the far run must give the compact case's result, while a
row product evaluated in 32 bits, or a byte offset kept in 32 bits, reads another location.

* far_map: the map.  Seams are the element offsets 2^29, 2^30, 2^31 (byte offsets 2^31, 2^32,
  2^33) and, for top = 2^32, 2^32.  Rows are dealt out by record-count class (1, 2-4, 5-16, more
  than 16, and "hot": at least 256), so that in every batch every class present has a row at or
  beyond the last seam and, where the class has a row for each seam, in the stretch after each
  earlier one.
* wrapped_reads: what a kernel with one of three addressing faults would read, from the model
  "mapped rows hold the case's parameters, everything else the padding value" alone.
* gather_rows / rows_differing: far tensors -> compact arrays, and the padding check.
* FarModel / FarOptimizer: the attributes TrainEngine reads of a model and an optimiser, around
  tensors made on the device (ReconstructInducer would draw A on the host for all n rows).
"""
import numpy as np

SEAMS = (2 ** 29, 2 ** 30, 2 ** 31, 2 ** 32)
TAIL = 64                   # rows after the one that holds element `top`
REPS = 32                   # rows kept for class representatives behind an earlier seam's five
HOT = 256                   # records from which a row is "hot" (the heavy-row chunks)
# (lo, hi) records of a batch: _grad_ref.ROW_CLASSES and the hot row
CLASSES = ((1, 1), (2, 4), (5, 16), (17, HOT - 1), (HOT, 1 << 30))
FAULTS = ("int32", "uint32", "byte32")
CHUNK_BYTES = 1 << 30       # the padding check's largest temporary (bool, one byte per element)


def seams_of(top):
    assert top in SEAMS[2:], top
    return tuple(S for S in SEAMS if S <= top)


def class_of(counts):
    """Class index of every count (-1: no record)."""
    counts = np.asarray(counts)
    out = np.full(counts.shape, -1, dtype=np.int64)
    for k, (lo, hi) in enumerate(CLASSES):
        out[(counts >= lo) & (counts <= hi)] = k
    return out


class FarMap:
    """rows[i]: the far row of compact id i; n_far rows of `width` elements; seam_rows[S] =
    floor(S / width), the row that straddles seam S whenever width does not divide S."""

    def __init__(self, rows, n_far, width, top):
        self.rows = np.asarray(rows, dtype=np.int64)
        self.n_far, self.width, self.top = int(n_far), int(width), int(top)
        self.seams = seams_of(top)
        self.seam_rows = {S: S // width for S in self.seams}

    def stretch(self, S):
        """[first, last) rows of the stretch that starts with seam S's row."""
        i = self.seams.index(S)
        end = self.seam_rows[self.seams[i + 1]] if i + 1 < len(self.seams) else self.n_far
        return self.seam_rows[S], end

    def rows_at(self, S):
        """How many compact ids are mapped into seam S's stretch."""
        lo, hi = self.stretch(S)
        return int(((self.rows >= lo) & (self.rows < hi)).sum())

    def inverse(self):
        """(sorted far rows, their compact ids)."""
        order = np.argsort(self.rows)
        return self.rows[order], order


def far_map(counts, width, top=2 ** 31):
    """counts: (batches, n) records of every compact row in every batch (a vector is one batch).
    Returns the FarMap of all n compact ids onto n_far = ceil(top / width) + TAIL rows:

    * for each seam S the rows floor(S / width) - 2 ... + 2 are used, the straddling row
      floor(S / width) first, and after the last seam every row up to n_far - 1;
    * in every batch, every class present has a row at or beyond the last seam, and a class
      with at least as many rows as there are seams also one in the stretch after each earlier
      seam (a class of fewer rows: as far as its unused ids go);
    * the other ids go round-robin to a block at row 0 and a block behind each earlier seam's
      five rows, each block filled from its far end: the map is not monotone."""
    counts = np.atleast_2d(np.asarray(counts, dtype=np.int64))
    n = counts.shape[1]
    seams = seams_of(top)
    n_far = -(-top // width) + TAIL
    k = {S: S // width for S in seams}
    cls = class_of(counts)
    rows = np.full(n, -1, dtype=np.int64)
    taken = set()

    def slots(S):       # the straddling row first, then outwards / onwards
        if S == seams[-1]:
            return [k[S]] + list(range(k[S] + 1, n_far)) + [k[S] - 1, k[S] - 2]
        return [k[S]] + list(range(k[S] + 1, k[S] + 3 + REPS)) + [k[S] - 1, k[S] - 2]

    free = {S: slots(S) for S in seams}

    def place(i, S):
        row = free[S].pop(0)
        assert rows[i] < 0 and row not in taken
        rows[i] = row
        taken.add(row)

    # class representatives: the last seam first (its rows are the scarce ones), the hot class
    # first, the heaviest unused id of the class (ids are in descending frequency: the lightest
    # are many)
    for S in reversed(seams):
        lo = k[S]
        hi = k[seams[seams.index(S) + 1]] if S != seams[-1] else n_far
        for c in reversed(range(len(CLASSES))):
            while any(r >= lo for r in free[S]):
                # batches whose class c has no row in this stretch yet; the unused id that is of
                # class c in most of them (the heaviest of those: the lightest are many)
                need = [b for b in range(counts.shape[0]) if np.any(cls[b] == c) and not
                        np.any((rows[cls[b] == c] >= lo) & (rows[cls[b] == c] < hi))]
                cover = (cls[need] == c).sum(axis=0) * (rows < 0) if need else np.zeros(n, int)
                if not cover.any():
                    break
                best = np.nonzero(cover == cover.max())[0]
                i = best[np.argmax(counts[need][:, best].sum(axis=0))]
                while free[S][0] < lo:                  # keep the rows before the seam for later
                    free[S].append(free[S].pop(0))
                place(int(i), S)
    # every listed row is used: fill what the representatives left
    rest = [int(i) for i in np.nonzero(rows < 0)[0]]
    for S in seams:
        while free[S] and rest:
            place(rest.pop(len(rest) // 2), S)
    # the bulk: round-robin over the blocks, each filled downwards
    bases = [0] + [k[S] + 3 + REPS for S in seams[:-1]]
    nblk = len(bases)
    size = -(-len(rest) // nblk)
    for S in seams[:-1]:
        assert k[S] + 3 + REPS + size <= k[seams[seams.index(S) + 1]] - 2, "block runs into the next seam"
    assert size <= k[seams[0]] - 2
    for j, i in enumerate(rest):
        row = bases[j % nblk] + size - 1 - j // nblk
        assert row not in taken
        rows[i] = row
    return FarMap(rows, n_far, width, top)


def check_map(fm, counts):
    """The properties the far tests rely on; returns a list of violations."""
    counts = np.atleast_2d(np.asarray(counts, dtype=np.int64))
    bad = []
    rows = fm.rows
    if rows.min() < 0 or rows.max() >= fm.n_far:
        bad.append("a row is out of range")
    if np.unique(rows).size != rows.size:
        bad.append("the map is not injective")
    d = np.diff(rows)
    if np.all(d > 0) or np.all(d < 0):
        bad.append("the map is monotone")
    if fm.n_far != -(-fm.top // fm.width) + TAIL:
        bad.append("n_far")
    if (fm.n_far - 1) * fm.width < fm.top or fm.n_far >= 2 ** 31:
        bad.append("the table does not pass the last seam (or has 2^31 rows)")
    used = set(rows.tolist())
    for S in fm.seams:
        kS = fm.seam_rows[S]
        if not all(kS + j in used for j in range(-2, 3)):
            bad.append(f"seam {S}: rows {kS - 2} ... {kS + 2} are not all used")   # straddling: kS
    if not all(r in used for r in range(fm.seam_rows[fm.top], fm.n_far)):
        bad.append("the last rows are not all used")
    if not all(r in used for r in range(3)):
        bad.append("row 0 and its neighbours are not used")
    cls = class_of(counts)
    for b in range(counts.shape[0]):
        for c in range(len(CLASSES)):
            ids = np.nonzero(cls[b] == c)[0]
            if ids.size == 0:
                continue
            for S in fm.seams:
                lo, hi = fm.stretch(S)
                # at or beyond EVERY seam: a row in the last stretch; a class with a row to
                # spare for each seam also in the stretch of every earlier one
                must = S == fm.top or ids.size >= len(fm.seams)
                if must and not np.any((rows[ids] >= lo) & (rows[ids] < hi)):
                    bad.append(f"batch {b}: class {CLASSES[c]} has no row in the stretch of {S}")
    return bad


# ------------------------------------------------------------------------------------------
# teeth: what an addressing fault would read
# ------------------------------------------------------------------------------------------
def _wrap(e, fault):
    e = np.asarray(e, dtype=np.int64)
    if fault == "int32":            # the element offset truncated to int32
        return ((e + 2 ** 31) % 2 ** 32) - 2 ** 31
    if fault == "uint32":           # ... to uint32
        return e % 2 ** 32
    if fault == "byte32":           # the byte offset kept modulo 2^32
        return e % 2 ** 30
    raise ValueError(fault)


def wrapped_reads(fm, table, pad, fault, whole_offset):
    """For every mapped row whose elements a `fault` moves: (compact ids, inside, same).
    table: (n, width) compact contents (row i lives at far row fm.rows[i]); every other row of
    the far table holds `pad`.  whole_offset: the fault applies to row * width + j (else to the
    row product alone, j added in 64 bits).  inside[i]: some moved element lands inside the
    table; same[i]: every moved element reads, from inside the table, the value the right
    location holds -- the fault would go unseen on that row."""
    table = np.asarray(table)
    n, w = table.shape
    assert w == fm.width and n == fm.rows.size
    srt, ids_of = fm.inverse()
    j = np.arange(w, dtype=np.int64)
    base = fm.rows[:, None] * w
    e = base + j[None, :]
    e2 = _wrap(e, fault) if whole_offset else _wrap(base, fault) + j[None, :]
    moved = e2 != e
    hit = np.nonzero(moved.any(axis=1))[0]
    e2, moved = e2[hit], moved[hit]
    inside = (e2 >= 0) & (e2 < fm.n_far * w)
    r2 = np.where(inside, e2 // w, 0)
    c2 = np.where(inside, e2 % w, 0)
    pos = np.clip(np.searchsorted(srt, r2), 0, n - 1)
    mapped = srt[pos] == r2
    val = np.where(mapped, table[ids_of[pos], c2], np.asarray(pad, dtype=table.dtype))
    same_el = inside & (val == table[hit])
    same = np.all(same_el | ~moved, axis=1)
    return hit, (inside & moved).any(axis=1), same


# ------------------------------------------------------------------------------------------
# device helpers (torch tensors; pinned on small CPU tensors by tests/test_far_rows_host.py)
# ------------------------------------------------------------------------------------------
def gather_rows(t, rows):
    """Rows `rows` (int64 array) of tensor t as a numpy array: index_select where t lives, then
    the download."""
    import torch
    idx = torch.as_tensor(np.asarray(rows, dtype=np.int64), device=t.device)
    return t.index_select(0, idx).cpu().numpy()


def scatter_rows(t, rows, values):
    """t[rows] = values (a numpy array, or a scalar), on t's device."""
    import torch
    idx = torch.as_tensor(np.asarray(rows, dtype=np.int64), device=t.device)
    if np.isscalar(values):
        t.index_fill_(0, idx, values)
    else:
        t.index_copy_(0, idx, torch.as_tensor(np.ascontiguousarray(values), device=t.device))


def rows_differing(t, pad, chunk_bytes=CHUNK_BYTES):
    """Sorted int64 array of the rows of t (rows along dim 0) with any element != pad (NaN
    counts as different), computed where t lives in chunks whose temporaries stay within
    chunk_bytes."""
    import torch
    n = t.shape[0]
    w = max(1, t[0].numel()) if n else 1
    step = max(1, chunk_bytes // w)
    out = []
    for lo in range(0, n, step):
        part = t[lo:lo + step].reshape(min(step, n - lo), -1)
        hit = (part != pad).any(dim=1).nonzero().flatten()
        if hit.numel():
            out.append((hit + lo).cpu().numpy())
        del part, hit
    return np.concatenate(out).astype(np.int64) if out else np.zeros(0, dtype=np.int64)


def padding_violations(t, pad, allowed):
    """Rows of t that differ from pad although they are not in `allowed` (an int64 array)."""
    return np.setdiff1d(rows_differing(t, pad), np.asarray(allowed, dtype=np.int64))


# ------------------------------------------------------------------------------------------
# the engine's model and optimiser, from device tensors
# ------------------------------------------------------------------------------------------
class _Decoder:
    def __init__(self, model_type):
        self.model_type = model_type


class FarModel:
    """What TrainEngine reads of a model: decoder.model_type, m, r, s, l, n, alpha, extended_reg,
    params / param_names / named_params()."""

    def __init__(self, dec, m, r, s, l, n, alpha, extended_reg, named):
        import rae_oracle as O
        self.decoder = _Decoder(dec)
        self.m, self.r, self.s, self.l, self.n = int(m), int(r), int(s), int(l), int(n)
        self.alpha, self.extended_reg = float(alpha), bool(extended_reg)
        self.param_names = list(O.param_names(dec))
        assert self.param_names[:2] == ["W", "Wb"] and set(named) == set(self.param_names)
        self.params = [named[k] for k in self.param_names]

    def named_params(self):
        return dict(zip(self.param_names, self.params))


class FarOptimizer:
    def __init__(self, name, accumulator):
        self.name = name
        self.accumulator = accumulator


def far_tensors(p0, maps, sizes, pads, dev, adagrad):
    """The parameters of a case on the device: tensor k has sizes.get(k, its compact rows) rows,
    filled with pads[k] (torch.full) and then p0[k]'s rows scattered through maps[k]; tensors
    without a map are uploaded as they are.  Returns (named, accumulators or None): zero
    accumulators of the same shapes, in p0's order."""
    import torch
    named, acc = {}, {}
    for key, v in p0.items():
        if key in maps:
            shape = (int(sizes[key]),) + v.shape[1:]
            t = torch.full(shape, float(pads[key]), dtype=torch.float32, device=dev)
            scatter_rows(t, maps[key], v)
        else:
            t = torch.as_tensor(v, device=dev).clone()
        named[key] = t
        if adagrad:
            acc[key] = torch.zeros_like(t)
    return named, (acc if adagrad else None)
