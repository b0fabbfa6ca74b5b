"""fp64 restatement of the objectives over sampled negatives, written from the definitions and not from the kernels;
torch on the CPU with autograd, so no gradient is derived by hand here.

Row r has label y = labels[r]; it is weighted iff 1 <= y < I (and r < nvalid, when given).  Its slots are the label (value v0) and
the live slots of its list — cand[r, :] (per-row lists, int [R, N]) or shared[:] (one list, int [S]); a slot is dead when it is empty
(< 0), at or past I, or equal to y.  v = rows[r] . table_used[c] + bias_used[c] - logq[c], item 0 the zero row of bias -1000.
  softplus(x) = max(x, 0) + log1p(exp(-|x|))
  softmax  l_r = -log(p_label + 1e-5), p the softmax over the label and the live slots      (tests/_cand_ce_ref.py's loss)
  bce      l_r = softplus(-v0) + sum_s softplus(v_s)
  bpr      l_r = (1 / n_r) sum_s softplus(v_s - v0);  n_r = 0: l_r = 0
  loss = g sum over the weighted rows of l_r / (W + 1e-5), W the number of weighted rows
The inputs are the arrays the kernels read, i.e. already rounded to their storage dtype (_cand_ce_ref.round_like)."""
import numpy as np
import torch

from tests._cand_ce_ref import round_like, slots, used  # noqa: F401  (round_like: for the callers)

FORMS = ("softmax", "bce", "bpr")


def softplus(x):
    return torch.clamp(x, min=0.0) + torch.log1p(torch.exp(-torch.abs(x)))


def sigmoid(x):
    """1 / (1 + exp(-x)) with the exponential of a non-positive argument only (numpy, for the closed forms of the tests)."""
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def row_ids(lists, r, y, I):
    """Item ids of row r's slots: the label first, then the live list slots in list order (repeats kept)."""
    lists = np.asarray(lists)
    return slots(lists[r] if lists.ndim == 2 else lists, y, I)[0]


def row_loss(v, form):
    """l_r from the row's values v (torch f64 [1 + n], the label first)."""
    if form == "softmax":
        return -torch.log(torch.softmax(v, 0)[0] + 1e-5)
    if form == "bce":
        return softplus(-v[0]) + softplus(v[1:]).sum()
    if form == "bpr":
        return softplus(v[1:] - v[0]).mean() if v.numel() > 1 else v.sum() * 0.0
    raise ValueError(form)


def reference(rows, table, bias, labels, lists, logq=None, form="bce", g=1.0, nvalid=None):
    """dict(loss, row_loss [R], d_rows [R, C], d_table [I, C] (row 0 zero), d_bias [I - 1], values: the rows' value vectors (numpy,
    None for a row of weight 0), ids: their item ids, weight).  lists: cand [R, N] or shared [S]."""
    rows_t = torch.tensor(np.asarray(rows, dtype=np.float64), requires_grad=True)
    table_t = torch.tensor(np.asarray(table, dtype=np.float64), requires_grad=True)
    bias_t = torch.tensor(np.asarray(bias, dtype=np.float64), requires_grad=True)
    labels = np.asarray(labels, dtype=np.int64)
    R, I = rows_t.shape[0], table_t.shape[0]
    keep = torch.ones((I, 1), dtype=torch.float64)
    keep[0] = 0.0
    tu = table_t * keep                                              # item 0: the zero row, no parameter
    bu = torch.cat([torch.tensor([-1000.0], dtype=torch.float64), bias_t])
    lq = torch.zeros(I, dtype=torch.float64) if logq is None else torch.tensor(np.asarray(logq, dtype=np.float64))
    nlive = R if nvalid is None else int(nvalid)
    terms, values, ids_of = [], [], []
    weight = 0
    for r in range(R):
        y = int(labels[r])
        if not (1 <= y < I and r < nlive):
            terms.append(torch.zeros((), dtype=torch.float64))
            values.append(None)
            ids_of.append(None)
            continue
        weight += 1
        ids = torch.tensor(row_ids(lists, r, y, I))
        v = tu[ids] @ rows_t[r] + bu[ids] - lq[ids]
        terms.append(row_loss(v, form))
        values.append(v.detach().numpy())
        ids_of.append(ids.numpy())
    terms = torch.stack(terms)
    loss = g * terms.sum() / (weight + 1e-5)
    d_rows, d_table, d_bias = (np.zeros(tuple(t.shape)) for t in (rows_t, table_t, bias_t))
    if loss.requires_grad:
        got = torch.autograd.grad(loss, (rows_t, table_t, bias_t), allow_unused=True)
        d_rows, d_table, d_bias = (z if x is None else x.numpy() for x, z in zip(got, (d_rows, d_table, d_bias)))
    return dict(loss=float(loss.detach()), row_loss=terms.detach().numpy(), d_rows=d_rows, d_table=d_table, d_bias=d_bias, values=values,
                ids=ids_of, weight=float(weight))
