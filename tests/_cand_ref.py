"""numpy references for the evaluation on candidate lists, written from the definition and not from the kernels:
the counter-based negative sampler, the value of a candidate, and the label's place among its candidates."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def mix32(h):
    """edgl_mix32 (the murmur3 finaliser) on uint32 values held in uint64 arrays."""
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def sampler_key(seed, step):
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    k = mix32((seed & 0xFFFFFFFF) ^ 0xC4ED1DA7)
    k = mix32((int(k) + (seed >> 32)) & 0xFFFFFFFF)
    return mix32(int(k) ^ (step & 0xFFFFFFFF))


def draw(k, row, slot, att, lo, hi):
    """The id of attempt `att` for (row, slot); row / slot / att broadcast."""
    row, slot, att = (np.asarray(a, dtype=np.uint64) for a in (row, slot, att))
    h = mix32(np.uint64(k) ^ mix32(row & M32))
    h = mix32((h + ((slot * np.uint64(0x9E3779B1)) & M32)) & M32)
    h = mix32(h ^ ((att * np.uint64(0x85EBCA6B)) & M32))
    return (np.uint64(lo) + ((h * np.uint64(hi - lo)) >> np.uint64(32))).astype(np.int64)


def sample_negatives(seen, labels, n, lo, hi, seed, step=0, row0=0):
    """(cand int32 [R, n], worst attempt count): the first of 32 attempts that is neither seen nor the label, else -1."""
    labels = np.asarray(labels)
    R = len(labels)
    k = sampler_key(seed, step)
    out = np.full((R, n), -1, dtype=np.int32)
    worst = 0
    slots = np.arange(n)
    for r in range(R):
        banned = {int(labels[r])} | (set(int(v) for v in seen[r]) if seen is not None else set())
        open_ = np.ones(n, dtype=bool)
        for att in range(32):
            if not open_.any():
                break
            ids = draw(k, row0 + r, slots, att, lo, hi)
            ok = open_ & ~np.isin(ids, list(banned))
            out[r, ok] = ids[ok]
            open_ &= ~ok
            worst = max(worst, att + 1)
    return out, worst


def chi2_uniform(ids, lo, hi, bins):
    cnt = np.bincount(((ids - lo) * bins // (hi - lo)).astype(np.int64), minlength=bins).astype(np.float64)
    e = len(ids) / bins
    return float(((cnt - e) ** 2 / e).sum())


def values(rows, table, bias, ids, seen, r):
    """(v, magnitude) in fp64 of the ids `ids` for row r: v = -inf for id < 0, id >= I and seen ids; the used table (row 0 zero, bias
    -1000 for item 0); magnitude = |b| + sum_k |x_k w_k| (the scale of the f32 rounding bound)."""
    I = table.shape[0]
    ids = np.asarray(ids, dtype=np.int64)
    ok = (ids >= 0) & (ids < I)
    c = np.where(ok, ids, 0)
    w = table[c].astype(np.float64)
    w[c == 0] = 0.0
    b = np.where(c == 0, -1000.0, bias.astype(np.float64)[np.maximum(c, 1) - 1])
    x = rows[r].astype(np.float64)
    v = w @ x + b
    mag = np.abs(w) @ np.abs(x) + np.abs(b)
    dead = ~ok
    if seen is not None:
        dead |= np.isin(ids, seen[r])
    v[dead] = -np.inf
    return v, mag


def count_before(v, vy, ids, y):
    """#{n : c >= 0, c != y, v_c > v_y or (v_c == v_y and c < y)}"""
    ids = np.asarray(ids, dtype=np.int64)
    return int(((ids >= 0) & (ids != y) & ((v > vy) | ((v == vy) & (ids < y)))).sum())


def reference(rows, table, bias, cand, seen, labels):
    """scores fp64 [R, N], label_val fp64 [R], count int [R], and the magnitudes of both (for the rounding bound)."""
    R, N = cand.shape
    sc, mg = np.empty((R, N)), np.empty((R, N))
    lv, lm, cnt = np.empty(R), np.empty(R), np.zeros(R, dtype=np.int64)
    for r in range(R):
        sc[r], mg[r] = values(rows, table, bias, cand[r], seen, r)
        if labels is not None:
            v, m = values(rows, table, bias, [labels[r]], seen, r)
            lv[r], lm[r] = v[0], m[0]
            cnt[r] = count_before(sc[r], lv[r], cand[r], int(labels[r]))
    return sc, lv, cnt, mg, lm


def rank_bracket(sc, mg, lv, lm, cand, labels, C):
    """[lo, hi] of the count that f32 rounding leaves open: an id is surely ahead / possibly ahead of the label by the bound
    (C + 2) 2^-24 magnitude on either value."""
    eps = (C + 2) * 2.0 ** -24
    lo, hi = [], []
    for r in range(len(labels)):
        ids, y = cand[r].astype(np.int64), int(labels[r])
        live = (ids >= 0) & (ids != y)
        a_lo, a_hi = sc[r] - eps * mg[r], sc[r] + eps * mg[r]
        y_lo, y_hi = lv[r] - eps * lm[r], lv[r] + eps * lm[r]
        sure = live & ((a_lo > y_hi) | ((sc[r] == -np.inf) & (lv[r] == -np.inf) & (ids < y)))
        maybe = live & ((a_hi >= y_lo) | ((sc[r] == -np.inf) & (lv[r] == -np.inf) & (ids < y)))
        lo.append(int(sure.sum()))
        hi.append(int(maybe.sum()))
    return np.array(lo), np.array(hi)
