"""float64 model of GRU4REC with --rnn_cell lstm: tests/_gru4rec_ref.py with the stacked GRU replaced by
torch.nn.LSTM(num_layers=L).double(), which IS cuDNN's LSTM; the canonical parts i | f | c | o go in transposed."""
import numpy as np
import torch

from tests import _seq_baselines_ref as SR
from tests._gru4rec_ref import BIAS, GRU_SCOPE, TABLE

GATES = ("i", "f", "c", "o")


def shapes(I, C, nb):
    s = {TABLE: (I, C), BIAS: (I - 1,)}
    for l in range(nb):
        for g in GATES:      # weights in tf.layers.dense orientation [in, out]
            s[GRU_SCOPE + f"{l}/w_{g}"] = s[GRU_SCOPE + f"{l}/r_{g}"] = (C, C)
            s[GRU_SCOPE + f"{l}/b_w{g}"] = s[GRU_SCOPE + f"{l}/b_r{g}"] = (C,)
    return s


def train(p, features, labels, C, nb, l2_reg):     # (loss, training logits [B*T, I], evaluation logits [B, I])
    ids = torch.as_tensor(np.asarray(features["seqs_i"]), dtype=torch.long)
    x = SR.zero_padded(p[TABLE])[ids] * (C ** 0.5)
    cat = lambda l, pre: torch.cat([p[GRU_SCOPE + f"{l}/{pre}{g}"] for g in GATES], dim=-1)
    w = {}
    for l in range(nb):
        w[f"weight_ih_l{l}"], w[f"weight_hh_l{l}"] = cat(l, "w_").t(), cat(l, "r_").t()
        w[f"bias_ih_l{l}"], w[f"bias_hh_l{l}"] = cat(l, "b_w"), cat(l, "b_r")
    h = torch.func.functional_call(torch.nn.LSTM(C, C, num_layers=nb, batch_first=True).double(), w, (x,))[0]
    rows = h * (ids != 0).to(x.dtype).unsqueeze(-1)
    logits = SR._logits(p, TABLE, BIAS, rows.reshape(-1, C))
    return SR.all_position_loss(logits, labels) + SR._l2(p, (TABLE,), l2_reg), logits, SR._logits(p, TABLE, BIAS, rows[:, -1])
