"""tests/_loopback.py's movers on CPU tensors against the semantics rae/dist.py documents and
tests/test_dist.py pins over gloo (test_exchange_all_gather_gloo, test_row_exchange_and_sync_gloo):
the same buffers, the same expected values, G = 2, 3, 4 -- once through the movers and once
through the ranks' ports (every rank enters, the last one moves the bytes)."""
import numpy as np
import pytest
import torch

from _loopback import Loopback, Ranks, refuse_p2p

WS = [2, 3, 4]


def _gather_bufs(G, n=5):
    bufs = []
    for rk in range(G):
        buf = torch.full((G * n,), -1.0)
        buf[rk * n:(rk + 1) * n] = torch.arange(n, dtype=torch.float32) + 100 * (rk + 1)
        bufs.append(buf)
    want = np.concatenate([np.arange(n, dtype=np.float32) + 100 * (k + 1) for k in range(G)])
    return bufs, want


def _rows_bufs(G):
    sends = [torch.arange(G * 3, dtype=torch.float32) + 1000 * rk for rk in range(G)]
    recvs = [torch.full_like(s, -1.0) for s in sends]
    want = [np.concatenate([np.arange(3 * k, 3 * k + 3, dtype=np.float32) + 1000 * j
                            for j in range(G)]) for k in range(G)]
    return sends, recvs, want


def _sync_bufs(G):
    """11 rows and 7 rows: counts G does not divide (G = 2, 3, 4)."""
    lists = []
    for rk in range(G):
        t2 = torch.full((11, 3), -1.0)
        t2[rk::G] = torch.arange(11, dtype=torch.float32)[rk::G, None] * 10 + rk
        t1 = torch.full((7,), -1.0)
        t1[rk::G] = torch.arange(7, dtype=torch.float32)[rk::G] + 0.5
        lists.append([t2, None, t1])
    t2 = np.arange(11, dtype=np.float32)[:, None] * 10 + (np.arange(11) % G)[:, None]
    return lists, np.repeat(t2, 3, axis=1), np.arange(7, dtype=np.float32) + 0.5


@pytest.mark.parametrize("G", WS)
@pytest.mark.parametrize("ports", [False, True], ids=["movers", "ports"])
def test_all_gather_slices(G, ports):
    bufs, want = _gather_bufs(G)
    lb = Loopback(G)
    if ports:
        for k in range(G):
            if k == G - 1:          # nothing has moved before the last rank enters
                assert float(bufs[0][-1]) == -1.0
            lb.port(k)(bufs[k])
    else:
        lb.gather(bufs)
    for buf in bufs:
        np.testing.assert_array_equal(buf.numpy(), want)


@pytest.mark.parametrize("G", WS)
@pytest.mark.parametrize("ports", [False, True], ids=["movers", "ports"])
def test_rows_block_k_of_rank_j_arrives_as_block_j_of_rank_k(G, ports):
    sends, recvs, want = _rows_bufs(G)
    lb = Loopback(G)
    if ports:
        for k in range(G):
            lb.port(k).rows(sends[k], recvs[k])
    else:
        lb.rows(sends, recvs)
    for k in range(G):
        np.testing.assert_array_equal(recvs[k].numpy(), want[k])
        np.testing.assert_array_equal(sends[k].numpy(), np.arange(G * 3, dtype=np.float32) + 1000 * k)


@pytest.mark.parametrize("G", WS)
@pytest.mark.parametrize("ports", [False, True], ids=["movers", "ports"])
def test_sync_rows_row_x_comes_from_rank_x_mod_G(G, ports):
    lists, want2, want1 = _sync_bufs(G)
    assert 11 % G and 7 % G
    lb = Loopback(G)
    if ports:
        for k in range(G):
            lb.port(k).sync_rows(lists[k])
    else:
        lb.sync_rows(lists)
    for t2, _, t1 in lists:
        np.testing.assert_array_equal(t2.numpy(), want2)
        np.testing.assert_array_equal(t1.numpy(), want1)


def test_ports_enter_once_in_rank_order():
    lb = Loopback(3)
    bufs, _ = _gather_bufs(3)
    lb.port(0)(bufs[0])
    with pytest.raises(RuntimeError):
        lb.port(2)(bufs[2])
    with pytest.raises(RuntimeError):
        lb.port(0)(bufs[0])


def test_max_int_answers_the_bound_and_keeps_what_was_asked():
    lb = Loopback(2)
    with pytest.raises(RuntimeError):
        lb.port(0).max_int(3)
    lb.bounds = (40, 90)
    got = [lb.port(0).max_int(7), lb.port(0).max_int(11), lb.port(1).max_int(5),
           lb.port(1).max_int(13), lb.port(0).max_int(8)]
    assert got == [40, 90, 40, 90, 40]
    assert lb.maxima == [(0, 0, 7), (0, 1, 11), (1, 0, 5), (1, 1, 13), (0, 0, 8)]
    assert lb.port(1).world_size == 2 and lb.port(1).rank == 1
    lb.port(0).barrier()
    with pytest.raises(RuntimeError):
        lb.port(0).all_gather_object({})


@pytest.mark.parametrize("xchg", ["p2p", "p2p_pipe"])
def test_peer_to_peer_is_refused_before_any_plan(xchg):
    made = []
    with pytest.raises(ValueError):
        Ranks(2, lambda rank, ex: made.append(rank), {"dp_xchg": xchg})
    assert not made
    refuse_p2p({"dp_xchg": "collective"})
    refuse_p2p(None)
