"""rae_neg_sample_philox on an MI355X, bit for bit: include/rae.h promises "Philox4x32-10 at
counter offset + i under key seed", and TrainEngine.eval_negatives relies on the offsets (neg2
starts at offset s N, any integer).  The draws must equal
    cum.searchsorted(u cum[-1]),  u = ((c0 >> 5) 2^26 + (c1 >> 6)) / 2^53
from the numpy restatement (tests/_entry_ref.py, pinned by the Random123 known answers in
tests/test_philox.py) at counter (lo32(idx), hi32(idx), 0, 0), idx = offset + i, key
(lo32(seed), hi32(seed)): a wrong multiplier, key schedule, word order or a lost carry of the
draw index into the counter's second word changes the draws."""
import ctypes as C

import numpy as np
import pytest

import _entry_ref as E

pytestmark = pytest.mark.gpu

#        (seed, offset, count): no count is a multiple of the 256-thread workgroup
STREAMS = [
    (0, 0, 5000),
    (0x5EEDE7A1, 0, 5000),                  # TrainEngine.EVAL_SEED
    ((1 << 63) + 12345, 7, 5000),           # high key word set
    (1, (1 << 32) - 5, 1000),               # the index carries into the counter's second word
    (1, (1 << 40) + 3, 1000),
]


def _cdfs():
    from rae.data import neg_sampling_cum
    g = np.random.RandomState(3)
    zipf = neg_sampling_cum(np.ceil(1e6 / np.arange(1, 20001)).astype(np.int64))
    mass = g.randint(1, 50, size=400).astype(np.float64)
    mass[g.choice(np.arange(1, 400), size=150, replace=False)] = 0.0     # runs of equal values
    mass[100:130] = 0.0
    runs = np.cumsum(mass) / mass.sum()
    return {"zipf20000": (zipf, None), "runs": (runs, mass), "n1": (np.array([1.0]), None)}


def _draw(lib, cum_t, seed, offset, count, dev):
    import torch
    from rae import _lib
    out = torch.full((count + 3,), -7, dtype=torch.int32, device=dev)
    _lib.check(lib.rae_neg_sample_philox(C.c_void_p(cum_t.data_ptr()), cum_t.numel(), seed, offset,
                                         count, C.c_void_p(out.data_ptr()), None))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[count:] == -7).all()
    return got[:count]


@pytest.mark.parametrize("cdf", ["zipf20000", "runs", "n1"])
def test_philox_stream_bit_for_bit(built_lib, cuda_dev, cdf):
    import torch
    cum, mass = _cdfs()[cdf]
    cum_t = torch.as_tensor(cum, device=cuda_dev)
    for seed, offset, count in STREAMS:
        assert count % 256 != 0
        got = _draw(built_lib, cum_t, seed, offset, count, cuda_dev)
        want = E.philox_draws(cum, seed, offset, count)
        assert np.array_equal(got, want), (cdf, hex(seed), offset,
                                           int((got != want).sum()), got[:8], want[:8])
        assert got.min() >= 0 and got.max() < len(cum)
        if mass is not None:
            assert (mass[got] > 0).all()            # zero-mass entries are never drawn
        if len(cum) == 1:
            assert (got == 0).all()
        else:
            assert len(np.unique(got)) > 50


def test_eval_negatives_offsets(built_lib, cuda_dev):
    """TrainEngine.eval_negatives: neg1 is the stream at offset 0, neg2 at offset s N (odd)."""
    from rae.data import synthetic_dataset
    from test_gpu_eval import _inducer
    s, N = 3, 211
    data, gold = synthetic_dataset(N, 300, 4, seed=8)
    ind = _inducer(data, gold, cuda_dev, "sp", 8, 16, s, 50)
    ind.compile_function()
    eng = ind.engine
    assert eng.split.N == N and (s * N) % 2 == 1
    n1, n2 = eng.eval_negatives(eng.split, ind.negativeSampler)
    cum = np.asarray(ind.negativeSampler.cum, dtype=np.float64)
    assert np.array_equal(n1.cpu().numpy(),
                          E.philox_draws(cum, eng.EVAL_SEED, 0, s * N).reshape(s, N))
    assert np.array_equal(n2.cpu().numpy(),
                          E.philox_draws(cum, eng.EVAL_SEED, s * N, s * N).reshape(s, N))
