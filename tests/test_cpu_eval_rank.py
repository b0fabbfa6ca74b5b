"""Evaluation by label rank (csrc/k_eval_rank.hip, Base.py:150-201), the parts that need no GPU: the host queries of the plan, the
refusals of every new entry point before any launch, the metric formulae the kernel must reproduce (metrics from a rank == metrics
from a top-K list), the driver flag and the sharded protocol (one SUM all-reduce of integer counts) under gloo."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

F32, BF16 = 0, 1
ONE = 16       # any non-null, 16-byte aligned address: the checks below fail before a pointer is dereferenced


def L():
    from easydgl_amd import _lib
    return _lib.lib


def err():
    return L().edgl_last_error().decode()


def test_host_queries_of_the_plan():
    lib = L()
    for C in (64, 128, 256):
        assert lib.edgl_score_rank_supported(512, C, 20001, 101, BF16) == 1
        assert lib.edgl_score_rank_supported(1, C, 1, 0, BF16) == 1              # no minimum of items, no K + T bound
        assert lib.edgl_score_rank_workspace(512, C, 20001, 101) >= 0
        assert lib.edgl_score_rank_slices(512, C, 20001, 101) >= 2
        assert lib.edgl_score_rank_supported(512, C, 20001, 101, F32) == 0
    for C in (32, 512):
        assert lib.edgl_score_rank_supported(512, C, 20001, 101, BF16) == 0
        assert lib.edgl_score_rank_workspace(512, C, 20001, 101) == -1
        assert lib.edgl_score_rank_slices(512, C, 20001, 101) == -1
    # bad arguments: rows, items (none, more than one call takes), seen width
    for R, n, T in ((0, 20001, 101), (512, 0, 101), (512, 262145, 101), (512, 20001, -1)):
        assert lib.edgl_score_rank_supported(R, 128, n, T, BF16) == 0
        assert lib.edgl_score_rank_workspace(R, 128, n, T) == -1
        assert lib.edgl_score_rank_slices(R, 128, n, T) == -1
    assert lib.edgl_score_rank_supported(512, 128, 262144, 201, BF16) == 1
    # a slice is bounded by its seen bitmap: 4096 items, 2048 at C = 256
    assert lib.edgl_score_rank_slices(512, 128, 262144, 201) >= 64
    assert lib.edgl_score_rank_slices(512, 256, 262144, 201) >= 128


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = L()
    # ---- label values of the fused form
    assert lib.edgl_score_label_value(None, ONE, ONE, ONE, 3, ONE, 8, 64, 100, ONE, BF16, None) == -4 and "null" in err()
    assert lib.edgl_score_label_value(ONE, ONE, ONE, ONE, 3, None, 8, 64, 100, ONE, BF16, None) == -4
    assert lib.edgl_score_label_value(ONE, ONE, ONE, None, 3, ONE, 8, 64, 100, ONE, BF16, None) == -4 and "seen" in err()
    assert lib.edgl_score_label_value(ONE, ONE, ONE, ONE, 3, ONE, 8, 64, 100, ONE, F32, None) == -2 and "bf16" in err()
    assert lib.edgl_score_label_value(ONE, ONE, ONE, ONE, 3, ONE, 8, 512, 100, ONE, BF16, None) == -1 and "{64, 128, 256}" in err()
    # ---- the counting sweep
    def fused(rows=ONE, table=ONE, bias=ONE, seen=ONE, T=3, labels=ONE, lv=ONE, R=8, C=64, I=1000, i0=0, i1=1000, count=ONE, dt=BF16):
        return lib.edgl_score_rank_fused(rows, table, bias, seen, T, labels, lv, R, C, I, i0, i1, count, None, dt, None)
    for kw in (dict(rows=None), dict(table=None), dict(bias=None), dict(labels=None), dict(lv=None), dict(count=None)):
        assert fused(**kw) == -4 and "null" in err(), kw
    assert fused(seen=None) == -4 and "seen" in err()
    assert fused(dt=F32) == -2 and "bf16" in err()
    assert fused(i0=4) == -1 and "bad item range [4, 1000) of 1000" in err()          # i0 % 8 != 0
    assert fused(i1=1001) == -1 and "bad item range [0, 1001) of 1000" in err()       # i1 > I
    assert fused(i0=8, i1=8) == -1 and "bad item range" in err()
    assert fused(C=512) == -1 and "{64, 128, 256}" in err()
    assert fused(I=300000, i1=300000) == -1 and "<= 262144 per call" in err()         # the bound is in the text
    assert fused(seen=8) == -1 and "16-byte" in err()
    # ---- tile form
    assert lib.edgl_label_value_tile(None, 4, 100, 0, ONE, 3, ONE, ONE, None) == -4 and "null" in err()
    assert lib.edgl_label_value_tile(ONE, 4, 100, 0, ONE, 3, None, ONE, None) == -4
    assert lib.edgl_label_value_tile(ONE, 4, 100, 0, ONE, 3, ONE, None, None) == -4
    assert lib.edgl_label_value_tile(ONE, 4, 100, 0, None, 3, ONE, ONE, None) == -4 and "seen" in err()
    assert lib.edgl_label_value_tile(ONE, 4, 100, 4, ONE, 3, ONE, ONE, None) == -1 and "i0 % 8" in err()
    assert lib.edgl_label_value_tile(ONE, 4, 0, 0, ONE, 3, ONE, ONE, None) == -1
    assert lib.edgl_rank_count_tile(None, 4, 100, 0, ONE, 3, ONE, ONE, ONE, None) == -4 and "null" in err()
    assert lib.edgl_rank_count_tile(ONE, 4, 100, 0, ONE, 3, ONE, None, ONE, None) == -4
    assert lib.edgl_rank_count_tile(ONE, 4, 100, 0, ONE, 3, ONE, ONE, None, None) == -4
    assert lib.edgl_rank_count_tile(ONE, 4, 100, 0, None, 3, ONE, ONE, ONE, None) == -4 and "seen" in err()
    assert lib.edgl_rank_count_tile(ONE, 4, 100, 12, ONE, 3, ONE, ONE, ONE, None) == -1 and "i0 % 8" in err()
    assert lib.edgl_rank_count_tile(ONE, 0, 100, 0, ONE, 3, ONE, ONE, ONE, None) == -1
    # ---- metrics from ranks
    assert lib.edgl_rank_metrics_from_rank(None, 4, ONE, 3, ONE, None) == -4 and "null" in err()
    assert lib.edgl_rank_metrics_from_rank(ONE, 4, None, 3, ONE, None) == -4
    assert lib.edgl_rank_metrics_from_rank(ONE, 4, ONE, 3, None, None) == -4
    assert lib.edgl_rank_metrics_from_rank(ONE, 4, ONE, 9, ONE, None) == -1 and "nk <= 8" in err()
    assert lib.edgl_rank_metrics_from_rank(ONE, 4, ONE, 0, ONE, None) == -1
    assert lib.edgl_rank_metrics_from_rank(ONE, 0, ONE, 3, ONE, None) == -1


def test_ops_refuse_cpu_tensors_and_bad_labels():
    from easydgl_amd import _lib, ops
    with pytest.raises(_lib.EdglError):
        ops.rank_from_logits(torch.zeros(2, 16), 0, None, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(_lib.EdglError):
        ops.rank_from_logits(torch.zeros(2, 16), 0, None, torch.zeros(2, dtype=torch.int32))        # labels are int64
    with pytest.raises(_lib.EdglError):
        ops.rank_metrics_from_rank(torch.zeros(2, dtype=torch.int32), torch.tensor([10], dtype=torch.int32), torch.zeros(4))


def metrics_from_rank(rank, ks):
    """The formulae of rank_metrics_from_rank_kernel: H@k = [rank < k], N@k = [rank < k] / log2(rank + 2), MRR = 1 / (rank + 1)."""
    rank = np.asarray(rank, dtype=np.int64)
    h = [float((rank < k).sum()) for k in ks]
    n = [float(((rank < k) / np.log2(rank + 2.0)).sum()) for k in ks]
    return h + n + [float((1.0 / (rank + 1.0)).sum())]


def test_metrics_from_rank_are_the_metrics_of_a_topk_list():
    """Base.py:181-201 on a top-K list (the label's position in the list, 0 when it is not in it) against the rank formulae."""
    rng = np.random.default_rng(3)
    I, R, K = 400, 300, 100
    rank = rng.integers(0, I, size=R)
    rank[:8] = (0, 9, 10, 49, 50, 99, 100, I - 1)
    label = rng.integers(0, I, size=R)
    lists = np.empty((R, K), dtype=np.int64)
    for r in range(R):          # any list of distinct items that holds the label at position rank[r] when rank[r] < K
        others = np.setdiff1d(rng.permutation(I)[:K + 1], [label[r]])[:K]
        lists[r] = others
        if rank[r] < K:
            lists[r, rank[r]] = label[r]
    want = np.zeros(6)
    for r in range(R):
        pos = np.where(lists[r] == label[r])[0]
        for i, k in enumerate((10, 50, 100)):
            if len(pos) and pos[0] < k:
                want[i] += 1.0
                want[3 + i] += 1.0 / np.log2(pos[0] + 2.0)
    got = metrics_from_rank(rank, (10, 50, 100))
    assert got[:3] == list(want[:3])
    np.testing.assert_allclose(got[3:6], want[3:], rtol=1e-12)
    # MRR and a cut-off beyond any list the top-K kernels build
    assert abs(metrics_from_rank([0, 1, 3], (500,))[-1] - (1 + 0.5 + 0.25)) < 1e-12
    assert metrics_from_rank([0, 499, 500], (500,))[0] == 2.0


def test_the_driver_knows_the_flag():
    from easydgl_amd import train
    base = ["--train", "a", "--valid", "b", "--test", "c", "--model", "EasyDGL", "--num_items", "10"]
    assert train.args(base).eval_by_rank is False
    assert train.args(base + ["--eval_by_rank"]).eval_by_rank is True
    import inspect
    assert inspect.signature(train.evaluate).parameters["by_rank"].default is False


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _np_rank(logits, seen, labels, i0, i1):
    """#{ j in [i0, i1), j != y : v_j > v_y or (v_j == v_y and j < y) } with the seen ids at -inf."""
    R = logits.shape[0]
    out = np.zeros(R, dtype=np.int32)
    for r in range(R):
        v = logits[r].astype(np.float64).copy()
        v[seen[r]] = -np.inf
        y = labels[r]
        j = np.arange(i0, i1)
        out[r] = int((((v[j] > v[y]) | ((v[j] == v[y]) & (j < y))) & (j != y)).sum())
    return out


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from easydgl_amd import parallel as P
    ok = True
    for n in (1003, 7):                                       # 7 rows: rank 1 holds an empty shard
        rng = np.random.default_rng(11)
        R = 6
        logits = rng.standard_normal((R, n)).astype(np.float32)
        logits[1, : n // 2] = 3.0                             # ties across the shard boundary
        seen = rng.integers(0, n, size=(R, 4))
        labels = rng.integers(0, n, size=R)
        labels[1], labels[2] = n // 3, seen[2, 0]             # inside the tie block; a seen label
        calls = []

        def count_local(i0, i1):
            calls.append((i0, i1))
            return torch.tensor(_np_rank(logits, seen, labels, i0, i1))

        got = P.sharded_rank(count_local, n, None)
        ok = ok and calls == [P.shard_bounds(n, world, rank)]
        if n == 7:
            ok = ok and (calls[0][1] - calls[0][0] == 0) == (rank == 1)
        ok = ok and got.dtype == torch.int32 and bool((got.numpy() == _np_rank(logits, seen, labels, 0, n)).all())
    out[rank] = ok
    dist.destroy_process_group()


def test_sharded_rank_world2_is_the_unsharded_rank():
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    assert all(out[r] for r in range(world)), dict(out)


def test_sharded_rank_single_process_is_the_local_count():
    from easydgl_amd import parallel as P
    c = P.sharded_rank(lambda i0, i1: torch.full((3,), i1 - i0, dtype=torch.int32), 10, None)
    assert c.tolist() == [10, 10, 10]
