"""Batch construction for the EasyDGL path — the semantics of the reference's MAUPostProcessor
(src/dataloader.py:159-206) without its per-example Python py_func (dataloader.py:34-36,183):
masked positions for a whole batch are drawn at once on the device."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch


def mask_last(tokens: torch.Tensor, timestamps: torch.Tensor, mask_id: int) -> Tuple[Dict[str, torch.Tensor], torch.Tensor]:
    """MAUPostProcessor.mask_last (dataloader.py:166-179): position T-1 := MASK, labels = the full sequence."""
    masked = tokens.clone()
    masked[:, -1] = mask_id
    return {"seqs_i": masked, "seqs_t": timestamps}, tokens


def draw_masked_positions(batch: int, seqslen: int, masklen: int, generator: torch.Generator = None,
                          device="cpu") -> torch.Tensor:
    """`masklen` DISTINCT positions in [1, seqslen) per row (np.random.choice(seqslen-1, masklen,
    replace=False) + 1, dataloader.py:34-36 with ignore_head = 1), vectorised: top-k of i.i.d. uniforms."""
    if masklen > seqslen - 1:
        raise ValueError("masklen must be <= seqslen - 1")
    u = torch.rand((batch, seqslen - 1), generator=generator, device=device)
    return (u.topk(masklen, dim=1).indices + 1).to(torch.int64)


def mask_random(tokens: torch.Tensor, timestamps: torch.Tensor, mask_id: int, masked_positions: torch.Tensor):
    """MAUPostProcessor.mask_random (dataloader.py:181-201)."""
    labels = tokens.gather(1, masked_positions)
    masked = tokens.scatter(1, masked_positions, mask_id)
    return {"seqs_i": masked, "seqs_t": timestamps, "masked_positions": masked_positions}, labels


def device_mask_random(tokens: torch.Tensor, timestamps: torch.Tensor, mask_id: int, masklen: int, rng_state: torch.Tensor,
                       stream_id: int = 0x4d41534b):
    """MAUPostProcessor.mask_random for a whole device batch in ONE kernel (edgl_mask_random): draws `masklen`
    distinct positions in [1, T) per row from the counter-based generator keyed on `rng_state` (uint64[2] = seed,
    step — advance the step between batches), replaces the tokens by MASK and gathers the labels."""
    from . import ops
    from ._lib import check, lib
    tokens = tokens.contiguous()
    B, T = tokens.shape
    masked = torch.empty_like(tokens)
    mpos = torch.empty((B, masklen), device=tokens.device, dtype=torch.int64)
    labels = torch.empty((B, masklen), device=tokens.device, dtype=torch.int64)
    check(lib.edgl_mask_random(ops._ptr(tokens), B, T, masklen, int(mask_id), ops._ptr(rng_state), stream_id,
                               ops._ptr(masked), ops._ptr(mpos), ops._ptr(labels), ops._stream()), "edgl_mask_random")
    return {"seqs_i": masked, "seqs_t": timestamps, "masked_positions": mpos}, labels


def device_mask_last(tokens: torch.Tensor, timestamps: torch.Tensor, mask_id: int):
    """MAUPostProcessor.mask_last on the device (edgl_mask_last)."""
    from . import ops
    from ._lib import check, lib
    tokens = tokens.contiguous()
    B, T = tokens.shape
    masked = torch.empty_like(tokens)
    check(lib.edgl_mask_last(ops._ptr(tokens), B, T, int(mask_id), ops._ptr(masked), ops._stream()), "edgl_mask_last")
    return {"seqs_i": masked, "seqs_t": timestamps}, tokens


LOADER_MODES = {"mask_random": 0, "mask_last": 1, "regressive_train": 2, "regressive_eval": 3}   # EDGL_LOADER_* of the header


class DeviceSplit:
    """A whole split (train / valid / test) resident in device memory: tokens int64 [N, T], times float32 [N, T], uploaded ONCE.
    The Netflix recipe's training split is ~180 MB; `nbytes(ids, ts)` is what the upload takes."""

    def __init__(self, ids, ts, device="cuda"):
        ids, ts = np.ascontiguousarray(ids, dtype=np.int64), np.ascontiguousarray(ts, dtype=np.float32)
        if ids.ndim != 2 or ids.shape != ts.shape or ids.shape[0] < 1 or ids.shape[1] < 2:
            raise ValueError(f"DeviceSplit: ids / ts must be [N >= 1, T >= 2] arrays of one shape (got {ids.shape} / {ts.shape})")
        if ids.shape[0] > 2 ** 31 - 1:
            raise ValueError("DeviceSplit: the permutation is int32: at most 2^31 - 1 sequences")
        self.tokens = torch.as_tensor(ids).to(device)
        self.times = torch.as_tensor(ts).to(device)
        self.N, self.T = int(ids.shape[0]), int(ids.shape[1])

    @staticmethod
    def nbytes(ids, ts) -> int:
        return int(np.prod(ids.shape)) * 8 + int(np.prod(ts.shape)) * 4

    def __len__(self):
        return self.N


class DeviceLoader:
    """Batches of a DeviceSplit, assembled by ONE kernel launch each (edgl_loader_batch) + a one-thread launch that advances the
    device-side (step, cursor) pair (edgl_loader_advance) — no host indexing, no host-to-device copy per batch.

    mode: "mask_random" (EasyDGL training: the draws of `device_mask_random` for the same (seed, step, stream_id), batch row by
    batch row), "mask_last" (EasyDGL evaluation), "regressive_train" / "regressive_eval" (`train.regressive_batch`).
    The host draws the epoch's order (`set_epoch(rng.permutation(N))`): batch k of the epoch holds rows perm[k*B : (k+1)*B], as on
    the host path.  The mask step counter runs on across epochs; `set_epoch` resets the cursor only.
    `full_batches` / `remainder` / `len()`: N // B, N % B and the steps of an epoch (the remainder batch counts as a step)."""

    def __init__(self, split: DeviceSplit, batch: int, mode: str = "mask_random", mask_id: int = 0, masklen: int = 0, seed: int = 0,
                 stream_id: int = 0x4d41534b):
        if mode not in LOADER_MODES:
            raise ValueError(f"DeviceLoader: unknown mode {mode!r} (one of {sorted(LOADER_MODES)})")
        if batch < 1:
            raise ValueError("DeviceLoader: batch must be >= 1")
        if mode == "mask_random" and not (1 <= masklen <= split.T - 1):
            raise ValueError("masklen must be in [1, seqslen - 1]")
        self.split, self.batch, self.mode, self.code = split, int(batch), mode, LOADER_MODES[mode]
        self.mask_id, self.masklen, self.stream_id = int(mask_id), int(masklen) if mode == "mask_random" else 0, int(stream_id)
        self.full_batches, self.remainder = divmod(split.N, self.batch)
        dev = split.tokens.device
        # { seed, step, cursor, reserved }: words 0..1 are the masker's rng_state (include/easydgl_hip.h)
        self.state = torch.tensor([int(seed), 0, 0, 0], dtype=torch.int64, device=dev)
        self.perm = None        # int32 [N] on the device once an order was set (None: identity, the kernel's NULL)
        self._pos = 0           # host mirror of the cursor: how many rows of the epoch were handed out (sizes next()'s batch)

    def __len__(self):
        return self.full_batches + (1 if self.remainder else 0)

    def remaining(self) -> int:
        """Rows of the epoch not handed out yet (host mirror of the device cursor)."""
        return max(self.split.N - self._pos, 0)

    def pin_order(self) -> None:
        """Give the order a device buffer of its own now (identity if none was set): a captured graph keeps its address."""
        if self.perm is None:
            self.perm = torch.arange(self.split.N, dtype=torch.int32, device=self.split.tokens.device)

    def set_epoch(self, perm=None) -> None:
        """Start an epoch: one small upload of the host-drawn order (None: identity) and a cursor reset."""
        N = self.split.N
        if perm is None:
            if self.perm is not None:
                self.perm.copy_(torch.arange(N, dtype=torch.int32, device=self.perm.device))
        else:
            perm = np.asarray(perm)
            if perm.shape != (N,):
                raise ValueError(f"DeviceLoader.set_epoch: the order must have {N} entries (got shape {perm.shape})")
            host = torch.as_tensor(perm.astype(np.int32))
            if self.perm is None:
                self.perm = host.to(self.split.tokens.device)
            else:
                self.perm.copy_(host)
        self.state[2:3].zero_()
        self._pos = 0

    def _shapes(self, count: int):
        T, M = self.split.T, self.masklen
        if self.mode == "mask_random":
            return (count, T), (count, M), (count, M)
        if self.mode == "mask_last":
            return (count, T), None, (count, T)
        return (count, T - 1), None, ((count, T - 1) if self.mode == "regressive_train" else (count, T))

    def write_into(self, seqs_i, seqs_t, mpos, labels, count: int = None) -> None:
        """Batch at the device cursor into the caller's buffers (row-major, at least `count` rows; default: a full batch), then the
        advance — two launches on the current stream, both capturable.  Rows past the end of the split come out empty."""
        from . import ops
        from ._lib import check, lib
        count = self.batch if count is None else int(count)
        si, mp, lb = self._shapes(count)
        for t, shape, dt, nm in ((seqs_i, si, torch.int64, "seqs_i"), (seqs_t, (count, self.split.T), torch.float32, "seqs_t"),
                                 (mpos, mp, torch.int64, "masked_positions"), (labels, lb, torch.int64, "labels")):
            if shape is None:
                continue
            if t is None or t.dtype != dt or t.dim() != 2 or t.shape[0] < shape[0] or t.shape[1] != shape[1]:
                raise ValueError(f"DeviceLoader.write_into: {nm} must be a {dt} tensor of at least {shape}")
        sp, st = self.split, ops._stream()
        check(lib.edgl_loader_batch(ops._ptr(sp.tokens), ops._ptr(sp.times), ops._ptr(self.perm), sp.N, sp.T, count, self.code,
                                    self.masklen, self.mask_id, ops._ptr(self.state), self.stream_id, ops._ptr(seqs_i), ops._ptr(seqs_t),
                                    ops._ptr(mpos) if mp is not None else None, ops._ptr(labels), st), "edgl_loader_batch")
        check(lib.edgl_loader_advance(ops._ptr(self.state), count, st), "edgl_loader_advance")
        if not torch.cuda.is_current_stream_capturing():
            self._pos += count

    def note_replay(self) -> None:
        """A captured pair of launches (a full batch) ran once more: keep the host mirror of the cursor in step."""
        self._pos += self.batch

    def next(self):
        """The next batch as FRESH tensors: (features, labels) as `device_mask_random` / `device_mask_last` /
        `train.regressive_batch` return them — a full batch, or what is left of the epoch (the remainder batch)."""
        count = min(self.batch, self.remaining())
        if count < 1:
            raise StopIteration("DeviceLoader.next: the epoch is exhausted (set_epoch starts the next one)")
        si, mp, lb = self._shapes(count)
        dev = self.split.tokens.device
        seqs_i = torch.empty(si, device=dev, dtype=torch.int64)
        seqs_t = torch.empty((count, self.split.T), device=dev, dtype=torch.float32)
        mpos = torch.empty(mp, device=dev, dtype=torch.int64) if mp is not None else None
        labels = torch.empty(lb, device=dev, dtype=torch.int64)
        self.write_into(seqs_i, seqs_t, mpos, labels, count)
        feats = {"seqs_i": seqs_i, "seqs_t": seqs_t}
        if mpos is not None:
            feats["masked_positions"] = mpos
        return feats, labels

    def cursor(self) -> int:
        """The device cursor (a synchronising read: tests and diagnostics)."""
        return int(self.state[2])


def synthetic_batch(num_items: int, seqslen: int, batch: int, seed: int = 9876, min_len: int = 5, ids: str = "zipf"):
    """SURVEY.md §8d synthetic sequences: row length ~ U{min_len..T}, left zero padding, Zipf(1.1) item ids
    clipped to [1, num_items-1], float32 timestamps 9.5e8 + cumsum(Exp(mean 3 days)).  T = seqslen + 1.
    (The clip piles ~35 % of the tokens on id num_items-1: `ids="uniform"` draws U[1, num_items) instead — no hot row, every
    gathered table row distinct with high probability: the variant that makes the embedding gather really read HBM.)"""
    ids_mode = ids
    rng = np.random.default_rng(seed)
    T = seqslen + 1
    ids = np.zeros((batch, T), dtype=np.int64)
    ts = np.zeros((batch, T), dtype=np.float32)
    lens = rng.integers(min(min_len, T), T + 1, size=batch)
    for b in range(batch):
        n = int(lens[b])
        ids[b, T - n:] = (rng.integers(1, num_items, size=n) if ids_mode == "uniform"
                          else np.clip(rng.zipf(1.1, size=n), 1, num_items - 1))
        ts[b, T - n:] = (9.5e8 + np.cumsum(rng.exponential(3 * 86400.0, size=n))).astype(np.float32)
    return ids, ts


def synthetic_mark_table(num_items: int, num_events: int, multi_hot: bool = False) -> np.ndarray:
    """[num_items, E] 0/1 table: mark (i mod E) for item i >= 1 (+ a second mark when multi_hot); row 0 = pad."""
    tab = np.zeros((num_items, num_events), dtype=np.uint8)
    idx = np.arange(1, num_items)
    tab[idx, idx % num_events] = 1
    if multi_hot:
        tab[idx, (idx * 7 + 3) % num_events] = 1
    return tab
