"""parallel.sum_over_ranks on CPU: a world-2 gloo group sums an int64 confusion matrix exactly (counts past 2^53, where a
detour through floating point would lose bits), leaves the input alone, and is the identity at world 1."""
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

K = 5


def _conf(rank):
    g = torch.Generator().manual_seed(7 + rank)
    c = torch.randint(0, 1 << 40, (K, K), generator=g, dtype=torch.int64)
    c[0, 0] = (1 << 60) + 1 + rank                  # not representable in float64
    return c


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank))
    import isa_amd  # noqa: F401
    from isa_amd import parallel as P
    assert P.init_from_env("gloo") == (world, rank, rank) and dist.is_initialized()
    mine = _conf(rank)
    total = P.sum_over_ranks(mine, world)
    assert torch.equal(mine, _conf(rank)), "the input must stay as it was"
    torch.save(dict(total=total, auto=P.sum_over_ranks(mine)), os.path.join(out_dir, "r%d.pt" % rank))
    dist.destroy_process_group()


def test_sum_over_ranks_world2(tmp_path):
    world, port = 2, 29747
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r = [torch.load(os.path.join(str(tmp_path), "r%d.pt" % i)) for i in range(world)]
    want = _conf(0) + _conf(1)
    assert int(want[0, 0]) == (1 << 61) + 3
    for i in range(world):
        assert r[i]["total"].dtype == torch.int64 and tuple(r[i]["total"].shape) == (K, K)
        assert torch.equal(r[i]["total"], want) and torch.equal(r[i]["auto"], want)


def test_sum_over_ranks_is_the_identity_at_world_1():
    import isa_amd  # noqa: F401
    from isa_amd import parallel as P
    c = _conf(0)
    assert P.sum_over_ranks(c, 1) is c and torch.equal(c, _conf(0))
    assert not dist.is_initialized() and P.sum_over_ranks(c) is c
