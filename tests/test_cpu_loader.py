"""Host side of the resident-split batch loader (csrc/k_data.hip edgl_loader_*, data.DeviceLoader): callable
without a GPU."""
import numpy as np
import pytest

NEW = ("edgl_loader_state_words", "edgl_loader_batch", "edgl_loader_advance")


def test_loader_symbols_are_declared_and_exported():
    from easydgl_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib, name), name
    assert _lib.lib.edgl_loader_state_words() == 4      # { seed, step, cursor, reserved }


def _batch(L, one, **kw):
    a = dict(tokens=one, times=one, perm=None, N=10, T=5, count=3, mode=0, M=2, mask_id=99, state=one, stream_id=1,
             seqs_i=one, seqs_t=one, mpos=one, labels=one)
    a.update(kw)
    return L.edgl_loader_batch(a["tokens"], a["times"], a["perm"], a["N"], a["T"], a["count"], a["mode"], a["M"], a["mask_id"],
                               a["state"], a["stream_id"], a["seqs_i"], a["seqs_t"], a["mpos"], a["labels"], None)


def test_entry_points_reject_bad_arguments_before_any_launch():
    from easydgl_amd import _lib
    L, one = _lib.lib, 16      # `one`: any aligned non-null address — the checks fail before a pointer is dereferenced
    for name in ("tokens", "times", "state", "seqs_i", "seqs_t", "labels", "mpos"):
        assert _batch(L, one, **{name: None}) == -4 and b"null pointer" in L.edgl_last_error(), name
    assert _batch(L, one, mode=1, mpos=None, T=1) == -1 and b"T >= 2" in L.edgl_last_error()      # (mask-last needs no positions)
    assert _batch(L, one, T=1) == -1 and b"T >= 2" in L.edgl_last_error()
    assert _batch(L, one, M=5) == -1 and b"masklen <= T-1" in L.edgl_last_error()                 # masklen > T - 1
    assert _batch(L, one, M=0) == -1 and b"masklen" in L.edgl_last_error()
    assert _batch(L, one, count=0) == -1 and b"count >= 1" in L.edgl_last_error()
    assert _batch(L, one, N=0) == -1 and b"N=0" in L.edgl_last_error()
    for mode in (-1, 4):
        assert _batch(L, one, mode=mode) == -1 and b"unknown mode" in L.edgl_last_error()
    assert _batch(L, one, T=20000, M=2) == -1 and b"too long" in L.edgl_last_error()
    assert L.edgl_loader_advance(None, 1, None) == -4 and b"null pointer" in L.edgl_last_error()
    assert L.edgl_loader_advance(one, 0, None) == -1 and b"count >= 1" in L.edgl_last_error()


@pytest.mark.parametrize("N,B,full,rem,steps", [(7, 3, 2, 1, 3), (150, 64, 2, 22, 3), (8, 4, 2, 0, 2), (3, 4, 0, 3, 1), (51200, 512, 100, 0, 100)])
def test_steps_per_epoch_and_remainder(N, B, full, rem, steps):
    """The split and the loader's bookkeeping live on whatever device the split is put on: the arithmetic needs no GPU."""
    from easydgl_amd import data as D
    ids = np.arange(N * 4, dtype=np.int64).reshape(N, 4)
    split = D.DeviceSplit(ids, np.zeros((N, 4), dtype=np.float32), device="cpu")
    assert len(split) == N and split.T == 4 and D.DeviceSplit.nbytes(ids, ids) == N * 4 * 12
    ld = D.DeviceLoader(split, B, "mask_random", mask_id=50, masklen=2, seed=7)
    assert (ld.full_batches, ld.remainder, len(ld)) == (full, rem, steps)
    assert ld.state.tolist() == [7, 0, 0, 0] and ld.remaining() == N
    ld.set_epoch(np.arange(N)[::-1])
    assert ld.perm.dtype.is_floating_point is False and ld.perm.tolist() == list(range(N - 1, -1, -1)) and ld.remaining() == N
    ld.note_replay()
    assert ld.remaining() == max(N - B, 0)
    ld.set_epoch(None)                                   # identity, written into the buffer the order already has
    assert ld.perm.tolist() == list(range(N)) and ld.remaining() == N


def test_loader_refuses_bad_construction():
    from easydgl_amd import data as D
    split = D.DeviceSplit(np.ones((5, 4), dtype=np.int64), np.zeros((5, 4), dtype=np.float32), device="cpu")
    with pytest.raises(ValueError, match="mode"):
        D.DeviceLoader(split, 2, "mask_first")
    with pytest.raises(ValueError, match="masklen"):
        D.DeviceLoader(split, 2, "mask_random", masklen=4)          # > T - 1
    with pytest.raises(ValueError, match="batch"):
        D.DeviceLoader(split, 0, "mask_last")
    with pytest.raises(ValueError, match="5 entries"):
        D.DeviceLoader(split, 2, "mask_last").set_epoch(np.arange(4))
    with pytest.raises(ValueError):
        D.DeviceSplit(np.ones((5, 1), dtype=np.int64), np.zeros((5, 1), dtype=np.float32), device="cpu")      # T < 2
    with pytest.raises(ValueError):
        D.DeviceSplit(np.ones((5, 4), dtype=np.int64), np.zeros((5, 3), dtype=np.float32), device="cpu")


def test_driver_parses_device_data():
    from easydgl_amd import train as TR
    base = ["--model", "EasyDGL", "--train", "a", "--valid", "b", "--test", "c", "--num_items", "10"]
    assert TR.args(base).device_data is False and TR.args(base).graph is False
    a = TR.args(base + ["--device_data", "--graph"])
    assert a.device_data is True and a.graph is True
