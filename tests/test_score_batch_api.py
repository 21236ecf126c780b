"""Batched score-only alignment, the parts that need no GPU: gsa_score_batch_dev in the header, the
library and the ctypes bindings, its argument check without a context, the Python entry points, and
the contract of the sharding adapter (shard.gpu_batch_score plugs into shard_align: scores back in
pair order), here with a CPU stand-in that scores every pair with the oracle.  The kernels are
checked in tests/test_gpu_score_batch.py."""
import ctypes
import inspect
import os
import re
import socket

import gpuseqalign_amd as gsa
from gpuseqalign_amd import shard
from tests._data import random_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO, GE = -11, -1


def test_entry_point_declared_exported_bound():
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    assert re.search(r"\bint\s+gsa_score_batch_dev\s*\(", text)
    assert hasattr(gsa.lib(), "gsa_score_batch_dev")
    res, args = gsa.SIGNATURES["gsa_score_batch_dev"]
    assert res is ctypes.c_int and len(args) == 11


def test_null_context_is_invalid_value():
    arr = (gsa.PairDev * 1)()
    out = (gsa.ScoreResult * 1)()
    ms = ctypes.c_float(0.0)
    st = gsa.lib().gsa_score_batch_dev(None, 1, arr, None, 25, GO, GE, 0, out, ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue


def test_python_entry_points_exist():
    for name, params in [("score_batch", ["pairs", "subst", "gapo", "gape", "local"]),
                         ("score_batch_dev", ["pairs", "subst_ptr", "substsz", "gapo", "gape", "local"])]:
        sig = inspect.signature(getattr(gsa.Engine, name))
        assert list(sig.parameters)[1:1 + len(params)] == params, name
    sig = inspect.signature(shard.gpu_batch_score)
    assert list(sig.parameters) == ["device", "gape", "local", "repeats", "warmup", "launch"]
    assert "gpu_batch_score" in shard.__all__
    assert callable(shard.gpu_batch_score())  # building the adapter touches no GPU


def _pairs():
    return [random_pair(r, c, 19 * r + c) for r, c in [(40, 50), (120, 30), (7, 9), (64, 64), (200, 150), (1, 5),
                                                       (90, 91), (33, 256), (150, 12)]]


def _oracle_scores(indices, pairs, subst, gapo):
    """An AlignBatchFn as shard.gpu_batch_score returns one: the "cost" per pair is its score."""
    import oracle
    return [int(oracle.score_ag(pairs[i][0], pairs[i][1], subst, gapo, GE, False)[0]) for i in indices], 0.002


def test_adapter_contract_world1(golden):
    import oracle
    assert callable(shard.gpu_batch_score(0, GE, False))  # the adapter this stand-in takes the place of
    pairs = _pairs()
    rep = shard.shard_align(pairs, golden.blosum62, GO, _oracle_scores)
    assert rep.world == 1
    assert [r.index for r in rep.results] == list(range(len(pairs)))
    assert [r.align_cost for r in rep.results] == [oracle.score_ag(y, x, golden.blosum62, GO, GE, False)[0]
                                                   for y, x in pairs]


def _worker(rank, world, port, subst, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rep = shard.shard_align(_pairs(), subst if rank == 0 else None, GO, _oracle_scores)
        q.put((rank, [(r.index, r.align_cost, r.rank) for r in rep.results], rep.world))
    finally:
        dist.destroy_process_group()


def test_adapter_contract_gloo_world2(golden):
    import oracle
    import torch.multiprocessing as mp
    assert callable(shard.gpu_batch_score(0, GE, False))  # (before any process starts)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, golden.blosum62, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    pairs = _pairs()
    expect = [oracle.score_ag(y, x, golden.blosum62, GO, GE, False)[0] for y, x in pairs]
    parts = shard.lpt_partition([(len(y) - 1) * (len(x) - 1) for y, x in pairs], 2)
    for rank, res, world in outs:
        assert world == 2
        assert [r[1] for r in res] == expect  # scores in pair order, on every rank
        for i, _, owner in res:
            assert i in parts[owner]
