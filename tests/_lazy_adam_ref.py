"""fp64 numpy reference of the lazy row-wise Adam (edgl_adam_rows): the touched set from the integer inputs and the
TF-form update on those rows.  No GPU, no torch."""
import numpy as np


def lr_t(lr, t, b1=0.9, b2=0.999):
    """Learning rate of Adam step t with both bias corrections folded in (tf.train.AdamOptimizer)."""
    return lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def touched_rows(I, ids=None, labels=None, cand=None):
    """bool [I]: row i in [1, I) is touched when it occurs in `ids`, is labels[r] of a row with 1 <= labels[r] < I, or is
    cand[r, n] of such a row.  Ids <= 0 or >= I are skipped; the list of a row of weight 0 touches nothing; row 0 never."""
    t = np.zeros(I, dtype=bool)

    def mark(x):
        x = np.asarray(x, dtype=np.int64).reshape(-1)
        t[x[(x >= 1) & (x < I)]] = True
    if ids is not None:
        mark(ids)
    if labels is not None:
        labels = np.asarray(labels, dtype=np.int64).reshape(-1)
        live = (labels >= 1) & (labels < I)
        mark(labels[live])
        if cand is not None:
            cand = np.asarray(cand, dtype=np.int64).reshape(labels.shape[0], -1)
            mark(cand[live])
    return t


def adam_all(w, g, m, v, t, lr, l2=0.0, b1=0.9, b2=0.999, eps=1e-8):
    """The plain TF-form Adam formula on every element (fp64): returns (w, m, v)."""
    w, g, m, v = (np.asarray(a, dtype=np.float64) for a in (w, g, m, v))
    g = g + l2 * w
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    return w - lr_t(lr, t, b1, b2) * m / (np.sqrt(v) + eps), m, v


def adam_rows(w, g, m, v, t, lr, ids=None, labels=None, cand=None, l2=0.0, b1=0.9, b2=0.999, eps=1e-8):
    """(w, m, v, g, touched) after one lazy step t on fp64 copies of [I, C] arrays: each touched row is updated exactly once,
    however often it is listed, and its gradient row reads zero afterwards; every other row is returned as it came."""
    w, g, m, v = (np.array(a, dtype=np.float64) for a in (w, g, m, v))
    t_rows = touched_rows(w.shape[0], ids, labels, cand)
    wn, mn, vn = adam_all(w[t_rows], g[t_rows], m[t_rows], v[t_rows], t, lr, l2, b1, b2, eps)
    w[t_rows], m[t_rows], v[t_rows] = wn, mn, vn
    g[t_rows] = 0.0
    return w, m, v, g, t_rows
