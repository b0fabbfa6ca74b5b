"""numpy references for the weighted negative sampler and the log-Q correction, written from the definition and not
from the kernels: the alias draw on top of tests/_cand_ref.py's counter-based words, the distribution a stored table implies, a
chi-square test against a target distribution, and the corrected loss as a bias shift of tests/_cand_ce_ref.py."""
import math

import numpy as np

from tests import _cand_ce_ref as CE
from tests import _cand_ref as CR

M32 = CR.M32
ALIAS_K = 0x68E31DA4          # the constant of the second word: h2 = mix32(h + K)


def attempt_word(k, row, slot, att):
    """The word h of attempt `att` for (row, slot): DESIGN 4.12's hashing, as in _cand_ref.draw."""
    row, slot, att = (np.asarray(a, dtype=np.uint64) for a in (row, slot, att))
    h = CR.mix32(np.uint64(k) ^ CR.mix32(row & M32))
    h = CR.mix32((h + ((slot * np.uint64(0x9E3779B1)) & M32)) & M32)
    return CR.mix32(h ^ ((att * np.uint64(0x85EBCA6B)) & M32))


def draw(k, row, slot, att, lo, hi, thr, alias):
    """The id of attempt `att`: bucket j = (h n) >> 32, h2 = mix32(h + K), id = lo + (h2 < thr[j] or alias[j] == j ? j : alias[j])."""
    h = attempt_word(k, row, slot, att)
    j = ((h * np.uint64(hi - lo)) >> np.uint64(32)).astype(np.int64)
    h2 = CR.mix32((h + np.uint64(ALIAS_K)) & M32)
    a = np.asarray(alias, dtype=np.int64)[j]
    t = np.asarray(thr, dtype=np.uint64)[j]
    return lo + np.where((h2 < t) | (a == j), j, a)


def sample_negatives(seen, labels, n, lo, hi, seed, thr, alias, step=0, row0=0):
    """(cand int32 [R, n], worst attempt count): _cand_ref.sample_negatives with the alias draw."""
    labels = np.asarray(labels)
    R = len(labels)
    k = CR.sampler_key(seed, step)
    out = np.full((R, n), -1, dtype=np.int32)
    worst = 0
    slots = np.arange(n)
    for r in range(R):
        banned = {int(labels[r])} | (set(int(v) for v in seen[r]) if seen is not None else set())
        open_ = np.ones(n, dtype=bool)
        for att in range(32):
            if not open_.any():
                break
            ids = draw(k, row0 + r, slots, att, lo, hi, thr, alias)
            ok = open_ & ~np.isin(ids, list(banned))
            out[r, ok] = ids[ok]
            open_ &= ~ok
            worst = max(worst, att + 1)
    return out, worst


def implied(thr, alias):
    """fp64 [n]: the probability of every bucket's id under a uniform bucket and a uniform 32-bit second word."""
    n = len(thr)
    alias = np.asarray(alias, dtype=np.int64)
    acc = np.where(alias == np.arange(n), 1.0, np.asarray(thr, dtype=np.float64) * 2.0 ** -32)
    p = acc.copy()
    np.add.at(p, alias, 1.0 - acc)
    return p / n


def chi2_sf(x, df):
    """P(chi^2_df > x): the regularised upper incomplete gamma function Q(df / 2, x / 2) by its series (x, df moderate)."""
    a, z = df / 2.0, x / 2.0
    if z <= 0.0:
        return 1.0
    term = total = 1.0 / a
    k = 0
    while abs(term) > 1e-17 * abs(total):
        k += 1
        term *= z / (a + k)
        total += term
    return 1.0 - total * math.exp(-z + a * math.log(z) - math.lgamma(a))


def chi2_quantile(q, df):
    lo, hi = 0.0, 10.0 * df + 100.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if 1.0 - chi2_sf(mid, df) < q:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def chi2_against(ids, lo, target, min_frac=1.0 / 50):
    """(chi^2, bins): the drawn ids against `target` (probabilities of lo, lo + 1, ..), neighbouring ids merged in ascending order
    until a bin expects at least min_frac of the draws (the last bin takes what is left)."""
    ids = np.asarray(ids).reshape(-1)
    N = len(ids)
    cnt = np.bincount(ids - lo, minlength=len(target)).astype(np.float64)
    obs, exp = [], []
    o = e = 0.0
    for c, p in zip(cnt, target):
        o += c
        e += p * N
        if e >= min_frac * N:
            obs.append(o); exp.append(e)
            o = e = 0.0
    if e > 0.0:
        obs[-1] += o; exp[-1] += e
    obs, exp = np.array(obs), np.array(exp)
    return float(((obs - exp) ** 2 / exp).sum()), len(obs)


def reference(rows, table, bias, logq, cand, labels, g=1.0):
    """The corrected loss is a bias shift: every logit v of item c >= 1 reads v - logq[c], item 0 keeps -1000 (logq[0] = 0)."""
    logq = np.asarray(logq, dtype=np.float64)
    return CE.reference(rows, table, np.asarray(bias, dtype=np.float64) - logq[1:], cand, labels, g)
