"""The resident-split batch kernel (csrc/k_data.hip loader_batch_kernel) against the host path it replaces — numpy indexing of
the split + data.device_mask_random / device_mask_last / train.regressive_batch — with torch.equal on every output.  The
output buffers are pre-filled with -1 / NaN, so an element the kernel leaves unwritten shows up."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MASK_ID = 777
SEED = 20240607

# (N, T, B, M): a whole epoch of 3 batches, the last with count 1 | only position 1 can be drawn | masklen = T - 1 |
# T above the 256 threads of a workgroup | the library's longest sequence
SHAPES = [(7, 5, 3, 2), (5, 2, 4, 1), (9, 33, 4, 32), (300, 257, 2, 10), (40, 1025, 2, 6)]


def _split(N, T, seed=0):
    from easydgl_amd import data as D
    rng = np.random.default_rng(seed)
    ids = rng.integers(1, 700, size=(N, T)).astype(np.int64)
    ids[rng.random((N, T)) < 0.2] = 0                      # some padding ids, anywhere
    ts = rng.random((N, T)).astype(np.float32) * 1e6 + 1.0
    return ids, ts, D.DeviceSplit(ids, ts)


def _host_batch(mode, ids, ts, rows, M, state):
    """What the host path hands the model for the source rows `rows` (train.py's loop), from the same (seed, step)."""
    from easydgl_amd import data as D
    from easydgl_amd import train as TR
    tok, tim = torch.as_tensor(ids[rows]).cuda(), torch.as_tensor(ts[rows]).cuda()
    if mode == "mask_random":
        return D.device_mask_random(tok, tim, MASK_ID, M, state[:2].clone())
    if mode == "mask_last":
        return D.device_mask_last(tok, tim, MASK_ID)
    return TR.regressive_batch(tok, tim, mode == "regressive_train")


def _buffers(ld, count):
    si, mp, lb = ld._shapes(count)
    i64 = lambda s: torch.full(s, -1, device="cuda", dtype=torch.int64)      # noqa: E731
    return (i64(si), torch.full((count, ld.split.T), float("nan"), device="cuda"), i64(mp) if mp is not None else None, i64(lb))


def _assert_batch(got_i, got_t, got_p, got_l, feats, labels, what):
    assert torch.equal(got_i, feats["seqs_i"]), what
    assert torch.equal(got_t, feats["seqs_t"]), what
    assert torch.equal(got_l, labels), what
    if got_p is not None:
        assert torch.equal(got_p, feats["masked_positions"]), what


@pytest.mark.parametrize("mode", ["mask_random", "mask_last", "regressive_train", "regressive_eval"])
@pytest.mark.parametrize("shape", SHAPES)
def test_epoch_equals_the_host_path(shape, mode):
    """A whole epoch under the reversed permutation: every batch (the short last one too) equals the host path's, and after
    each call plus advance `step` moved by 1 and `cursor` by count."""
    from easydgl_amd import data as D
    N, T, B, M = shape
    ids, ts, split = _split(N, T, seed=N)
    if mode != "mask_random" and N * T > 20000:
        N = 3 * B + 1                                       # the copy modes have no T-dependent path beyond the thread loop
        ids, ts = ids[:N], ts[:N]
        split = D.DeviceSplit(ids, ts)
    ld = D.DeviceLoader(split, B, mode, MASK_ID, M, SEED)
    perm = np.arange(N)[::-1].copy()
    ld.set_epoch(perm)
    nb = min(len(ld), 4)                                    # (the large splits: four batches, the cursor is the same code)
    lo = 0
    for k in range(nb):
        count = min(B, N - lo)
        state = ld.state.clone()
        assert state.tolist() == [SEED, k, lo, 0]
        bufs = _buffers(ld, count)
        ld.write_into(*bufs, count)
        feats, labels = _host_batch(mode, ids, ts, perm[lo:lo + count], M, state)
        _assert_batch(*bufs, feats, labels, (shape, mode, k))
        lo += count
    assert ld.state.tolist() == [SEED, nb, lo, 0] and ld.remaining() == N - lo
    if mode == "mask_random":
        mp = bufs[2]
        assert int(mp.min()) >= 1 and int(mp.max()) <= T - 1
        assert all(len(set(r.tolist())) == M for r in mp)


def test_next_returns_fresh_batches_and_the_remainder():
    from easydgl_amd import data as D
    N, T, B, M = 7, 5, 3, 2
    ids, ts, split = _split(N, T, seed=1)
    ld = D.DeviceLoader(split, B, "mask_random", MASK_ID, M, SEED)
    for epoch in range(2):                                  # the mask step counter runs on across epochs; the cursor restarts
        perm = np.random.default_rng(epoch).permutation(N)
        ld.set_epoch(perm)
        for k, lo in enumerate(range(0, N, B)):
            state = ld.state.clone()
            assert state.tolist() == [SEED, epoch * 3 + k, lo, 0]
            feats, labels = ld.next()
            want_f, want_l = _host_batch("mask_random", ids, ts, perm[lo:lo + B], M, state)
            assert labels.shape[0] == min(B, N - lo)
            _assert_batch(feats["seqs_i"], feats["seqs_t"], feats["masked_positions"], labels, want_f, want_l, (epoch, k))
        with pytest.raises(StopIteration):
            ld.next()


def test_identity_permutation_is_null():
    from easydgl_amd import data as D
    N, T, B, M = 9, 33, 4, 5
    ids, ts, split = _split(N, T, seed=2)
    for mode in ("mask_random", "regressive_eval"):
        ld = D.DeviceLoader(split, B, mode, MASK_ID, M, SEED)
        ld.set_epoch(None)
        assert ld.perm is None                              # the kernel's NULL
        ld.next()
        state = ld.state.clone()
        feats, labels = ld.next()
        want_f, want_l = _host_batch(mode, ids, ts, np.arange(4, 8), M, state)
        _assert_batch(feats["seqs_i"], feats["seqs_t"], feats.get("masked_positions"), labels, want_f, want_l, mode)


def test_one_source_row_twice_in_a_batch_gets_two_masks():
    """The key depends on the BATCH row, not on the source row: a permutation that names row 3 twice in one batch gives two
    output rows with different draws — exactly the host path's, which masks the gathered batch."""
    from easydgl_amd import data as D
    N, T, B, M = 6, 33, 4, 8
    ids, ts, split = _split(N, T, seed=3)
    ld = D.DeviceLoader(split, B, "mask_random", MASK_ID, M, SEED)
    perm = np.array([3, 1, 3, 0, 2, 5])
    ld.set_epoch(perm)
    state = ld.state.clone()
    feats, labels = ld.next()
    want_f, want_l = _host_batch("mask_random", ids, ts, perm[:4], M, state)
    _assert_batch(feats["seqs_i"], feats["seqs_t"], feats["masked_positions"], labels, want_f, want_l, "dup")
    mp = feats["masked_positions"]
    assert not torch.equal(mp[0], mp[2]) and not torch.equal(feats["seqs_i"][0], feats["seqs_i"][2])
    assert torch.equal(feats["seqs_t"][0], feats["seqs_t"][2])


@pytest.mark.parametrize("mode", ["mask_random", "mask_last", "regressive_train", "regressive_eval"])
def test_rows_past_the_end_come_out_empty(mode):
    """A full-batch call with 2 rows left (what a captured launch does when the caller replays once too often), a call with the
    cursor already past N, and a permutation entry outside [0, N): ids 0, times 0, labels 0, valid distinct positions."""
    from easydgl_amd import data as D
    N, T, B, M = 6, 9, 4, 3
    ids, ts, split = _split(N, T, seed=4)
    ld = D.DeviceLoader(split, B, mode, MASK_ID, M, SEED)
    perm = np.array([5, 4, 3, 2, 1, 0])
    ld.set_epoch(perm)
    ld.next()
    state = ld.state.clone()
    bufs = _buffers(ld, B)
    ld.write_into(*bufs)                                     # rows 4, 5 real, rows 6, 7 past the end
    got_i, got_t, got_p, got_l = bufs
    feats, labels = _host_batch(mode, ids, ts, perm[4:6], M, state)
    _assert_batch(got_i[:2], got_t[:2], None if got_p is None else got_p[:2], got_l[:2], feats, labels, mode)

    def empty(rows_i, rows_t, rows_p, rows_l):
        assert int(rows_i.abs().max()) == 0 and float(rows_t.abs().max()) == 0.0 and int(rows_l.abs().max()) == 0
        if rows_p is not None:
            assert int(rows_p.min()) >= 1 and int(rows_p.max()) <= T - 1
            assert all(len(set(r.tolist())) == M for r in rows_p)
    empty(got_i[2:], got_t[2:], None if got_p is None else got_p[2:], got_l[2:])
    assert ld.state.tolist() == [SEED, 2, 8, 0]              # the advance is unconditional: cursor = 8 > N
    bufs = _buffers(ld, B)
    ld.write_into(*bufs)                                     # cursor past N: all empty
    empty(*bufs)
    # a permutation entry outside [0, N) is an empty row too, the others are untouched by it
    ld.perm.copy_(torch.tensor([5, -1, 6, 2, 1, 0], dtype=torch.int32))
    ld.state[2:3].zero_()
    state = ld.state.clone()
    bufs = _buffers(ld, B)
    ld.write_into(*bufs)
    got_i, got_t, got_p, got_l = bufs
    empty(got_i[1:3], got_t[1:3], None if got_p is None else got_p[1:3], got_l[1:3])
    assert torch.equal(got_t[0], split.times[5]) and torch.equal(got_t[3], split.times[2])


def test_the_masker_itself_is_unchanged():
    """edgl_mask_random now calls the shared key / rank functions: same draws as the definition, restated on the host —
    the M smallest (key, position) of a counter-based hash of (seed, step, stream, row, position)."""
    from easydgl_amd import data as D
    B, T, M, stream = 5, 37, 7, 0x4d41534b
    seed, step = 0x123456789ab, 5
    ids, ts, _ = _split(B, T, seed=5)
    state = torch.tensor([seed, step], dtype=torch.int64, device="cuda")
    feats, labels = D.device_mask_random(torch.as_tensor(ids).cuda(), torch.as_tensor(ts).cuda(), MASK_ID, M, state, stream)
    m32 = 0xFFFFFFFF

    def mix(x):      # edgl_mix32 (edgl_common.h): the murmur3 finaliser
        x ^= x >> 16; x = (x * 0x85ebca6b) & m32; x ^= x >> 13; x = (x * 0xc2b2ae35) & m32; x ^= x >> 16
        return x
    k0 = mix(((seed & m32) ^ ((stream * 0x9E3779B9) & m32) ^ 0xA511E9B3) & m32)
    k1 = mix((((seed >> 32) & m32) + ((step & m32) * 0x85ebca6b) + ((step >> 32) & m32) + stream) & m32)
    want_pos = np.zeros((B, M), dtype=np.int64)
    for b in range(B):
        keys = []
        for t in range(1, T):
            h = ((((b * T + t) ^ k0) & m32) * 0x9E3779B1 + k1) & m32
            h ^= h >> 15; h = (h * 0x85ebca6b) & m32; h ^= h >> 13; h = (h * 0xc2b2ae35) & m32; h ^= h >> 16
            keys.append((h, t))
        want_pos[b] = [t for _, t in sorted(keys)[:M]]
    assert np.array_equal(feats["masked_positions"].cpu().numpy(), want_pos)
    want_i = ids.copy()
    np.put_along_axis(want_i, want_pos, MASK_ID, axis=1)
    assert np.array_equal(feats["seqs_i"].cpu().numpy(), want_i)
    assert np.array_equal(labels.cpu().numpy(), np.take_along_axis(ids, want_pos, axis=1))
