"""fp64 numpy reference of the sampled-softmax cross-entropy, written from the definition and not from the kernels.

Row r (label y = labels[r]) is scored against the slots {y} + cand[r, :]; a list slot is dead when it is empty (-1), at or past I,
or equal to y (accidental hit).  v = rows[r] . table_used[c] + bias_used[c] with item 0 the zero row of bias -1000.
  loss = sum_r w_r (-log(p_y + 1e-5)) / (sum w + 1e-5),   w_r = [y != 0],   p = softmax over the label and the live slots
The inputs are the arrays the kernel reads, i.e. already rounded to its storage dtype (round_like)."""
import numpy as np


def round_like(a, mode):
    """`a` rounded to the kernel's storage dtype ("f32" / "bf16"), as fp64."""
    import torch
    t = torch.as_tensor(np.asarray(a, dtype=np.float64))
    t = t.to(torch.bfloat16 if mode == "bf16" else torch.float32)
    return t.double().numpy()


def used(table, bias):
    tu = np.array(table, dtype=np.float64)
    tu[0] = 0.0
    return tu, np.concatenate([[-1000.0], np.asarray(bias, dtype=np.float64)])


def slots(cand_row, y, I):
    """Item ids of the row's slots: the label first, then the live list slots in list order (repeats kept)."""
    c = np.asarray(cand_row, dtype=np.int64)
    live = (c >= 0) & (c < I) & (c != y)
    return np.concatenate([[y], c[live]]), live


def reference(rows, table, bias, cand, labels, g=1.0):
    """dict(loss, lse [R], d_rows [R, C], d_table [I, C], d_bias [I - 1], terms [R]: w_r (-log(p_y + 1e-5)), weight)."""
    rows = np.asarray(rows, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    R, C = rows.shape
    I = table.shape[0]
    tu, bu = used(table, bias)
    weight = float((labels != 0).sum())
    W = weight + 1e-5
    lse, terms = np.zeros(R), np.zeros(R)
    d_rows, d_table, d_bu = np.zeros((R, C)), np.zeros((I, C)), np.zeros(I)
    for r in range(R):
        y = int(labels[r])
        if y == 0:
            continue
        ids, _ = slots(cand[r], y, I)
        v = tu[ids] @ rows[r] + bu[ids]
        m = v.max()
        lse[r] = m + np.log(np.exp(v - m).sum())
        p = np.exp(v - lse[r])
        terms[r] = -np.log(p[0] + 1e-5)
        coef = (1.0 / W) * p[0] / (p[0] + 1e-5)
        dv = g * coef * p
        dv[0] -= g * coef
        d_rows[r] = dv @ tu[ids]
        np.add.at(d_table, ids, dv[:, None] * rows[r][None, :])
        np.add.at(d_bu, ids, dv)
    d_table[0] = 0.0                 # item 0 is no parameter: the used table's zero row
    return dict(loss=g * terms.sum() / W, lse=lse, d_rows=d_rows, d_table=d_table, d_bias=d_bu[1:], terms=terms, weight=weight)


def loss_only(rows, table, bias, cand, labels):
    return reference(rows, table, bias, cand, labels)["loss"]


def full_softmax(rows, table, bias, labels):
    """The plain full-catalogue cross-entropy of the training paths (EasyDGL.py:149-155,177-185) in fp64, written with dense
    matrices: loss, d_rows, d_table (row 0 zero), d_bias."""
    rows = np.asarray(rows, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    tu, bu = used(table, bias)
    R = rows.shape[0]
    logits = rows @ tu.T + bu
    logits -= logits.max(axis=1, keepdims=True)
    p = np.exp(logits)
    p /= p.sum(axis=1, keepdims=True)
    w = (labels != 0).astype(np.float64)
    W = w.sum() + 1e-5
    py = p[np.arange(R), labels]
    loss = (w * -np.log(py + 1e-5)).sum() / W
    coef = (w / W) * py / (py + 1e-5)
    dl = p.copy()
    dl[np.arange(R), labels] -= 1.0
    dl *= coef[:, None]
    d_table = dl.T @ rows
    d_table[0] = 0.0
    return dict(loss=loss, d_rows=dl @ tu, d_table=d_table, d_bias=dl.sum(axis=0)[1:])
