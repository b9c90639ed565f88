"""CPU, world_size 2 over gloo: ranks that each accumulated the same views hold float atomic sums that differ in their last bits; a
cut at the k-th largest of them could keep different rows per rank.  ``ContributionStats.broadcast_`` (what ``harness.train`` calls
before it prunes with ``world_size`` > 1) makes every rank select on rank 0's sums: the same rows everywhere."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from fdgs.importance import ContributionStats
    P = 4000
    g = torch.Generator().manual_seed(0)
    # scores a rounding error apart from their neighbours, as the summed weights of a large model are
    exact = 100.0 * (1.0 + 2e-7 * torch.arange(P, dtype=torch.float64)[torch.randperm(P, generator=g)])
    noise = 1.0 + 3e-7 * torch.randn(P, generator=torch.Generator().manual_seed(100 + rank), dtype=torch.float64)
    st = ContributionStats(P, "cpu")
    st.weight_sum = (exact * noise).float()      # this rank's draw of the summation noise
    st.hits.fill_(1)
    mine = st.keep_mask(keep_fraction=0.5)
    both = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(both, mine)
    differ_before = not torch.equal(both[0], both[1])
    assert st.broadcast_(0) is st
    after = st.keep_mask(keep_fraction=0.5)
    both_after = [torch.zeros_like(after) for _ in range(world)]
    dist.all_gather(both_after, after)
    assert torch.equal(both_after[0], both_after[1]) and torch.equal(both_after[0], both[0])   # everybody keeps what rank 0 decided
    q.put((rank, differ_before, int(after.sum())))
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_ranks_keep_the_same_rows_after_the_broadcast_world2():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    res = sorted(q.get(timeout=10) for _ in range(world))
    assert res[0][1] and res[1][1], "the ranks' own sums selected the same rows: the test shows nothing"
    assert res[0][2] == res[1][2] >= 2000


def test_the_training_loop_broadcasts_before_it_prunes():
    """harness.train with world_size > 1 takes rank 0's sums between accumulate and prune_by_contribution."""
    import inspect
    from fdgs import harness
    src = inspect.getsource(harness.train)
    a, b, c = src.index("accumulate(model, cameras"), src.index("cstats.broadcast_(0)"), src.index("prune_by_contribution(model, optimizer, cstats")
    assert a < b < c and "if world_size > 1:" in src[a:b]
