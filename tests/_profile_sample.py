"""Shared by tests/test_profile_host.py and tests/test_gpu_profile.py: the reference's sample
input (tests/golden/data-sample.txt.gz) through rae.preprocess into a DatasetManager that keeps
its feature lexicon, and the row generators of the key-count tests."""
import functools
import gzip
import os
import shutil
import tempfile

import numpy as np

from conftest import GOLDEN

SAMPLE = os.path.join(GOLDEN, "data-sample.txt.gz")


@functools.lru_cache(maxsize=1)
def sample_data():
    """(DatasetManager with .featureLex, gold standard) of the sample, as `python -m
    rae.preprocess` followed by rae.preprocess.load_data gives them."""
    from rae import preprocess as P
    with tempfile.TemporaryDirectory() as tmp:
        plain = os.path.join(tmp, "data-sample.txt")
        with gzip.open(SAMPLE, "rb") as src, open(plain, "wb") as dst:
            shutil.copyfileobj(src, dst)
        out = os.path.join(tmp, "ds.json.gz")
        P.preprocess(plain, out)
        return P.load_data(out)


def zipf_ints(g, n, size, a=1.0):
    """Truncated Zipf(a) draws in [0, n), rank 0 the most frequent."""
    w = 1.0 / np.power(np.arange(1, n + 1, dtype=np.float64), a)
    cdf = np.cumsum(w)
    cdf /= cdf[-1]
    return np.searchsorted(cdf, g.random_sample(size), side="right").clip(0, n - 1)


def count_rows(g, n, m, nk, kind):
    """(labels int64, keys int32) of n rows: 'uniform', 'zipf' (Zipf keys, uniform labels),
    'one-cell', 'one-cluster' (Zipf keys in one cluster); ~2 % of the labels are -1 or m and
    ~2 % of the keys -1 or nk (skipped rows), except in 'one-cell'."""
    lab = g.randint(0, m, n).astype(np.int64)
    key = g.randint(0, nk, n).astype(np.int32)
    if kind in ("zipf", "one-cluster"):
        key = zipf_ints(g, nk, n).astype(np.int32)
    if kind == "one-cluster":
        lab[:] = m // 2
    if kind == "one-cell":
        lab[:] = m - 1
        key[:] = nk // 3
        return lab, key
    u, v = g.rand(n), g.rand(n)
    lab[u < 0.01] = -1
    lab[u > 0.99] = m
    key[v < 0.01] = -1
    key[v > 0.99] = nk
    return lab, key
