"""float64 torch restatement of GRU4REC from the formulas of src/model/GRU4REC.py: scaled zero-padded item embedding, num_blocks
cuDNN-form GRU layers in sequence (each reads the previous one's unmasked states), row mask, tied scoring, cross-entropy, l2 of the table."""
import numpy as np
import torch

from tests import _seq_baselines_ref as SR

GRU_SCOPE = "S2PNM/Reccurency/GRU4REC/GRU/opaque_kernel/"     # (the reference builds the blob under S2PNM's scope, GRU4REC.py:43)
TABLE, BIAS = "GRU4REC/item_embs/lookup_table", "GRU4REC/output_bias"


def gru4rec_shapes(I, C, nb):
    s = {TABLE: (I, C), BIAS: (I - 1,)}
    for l in range(nb):
        for g in SR.GRU_GATES:      # weights in tf.layers.dense orientation [in, out]
            s[GRU_SCOPE + f"{l}/w_{g}"] = s[GRU_SCOPE + f"{l}/r_{g}"] = (C, C)
            s[GRU_SCOPE + f"{l}/b_w{g}"] = s[GRU_SCOPE + f"{l}/b_r{g}"] = (C,)
    return s


def layer_parts(p, l):
    return tuple(torch.cat([p[GRU_SCOPE + f"{l}/{pre}{g}"] for g in SR.GRU_GATES], dim=-1) for pre in ("w_", "b_w", "r_", "b_r"))


def stacked_gru(p, x, nb):
    for l in range(nb):
        x = SR.gru(x, *layer_parts(p, l))
    return x


def gru4rec_rows(p, seqs_i, C, nb):
    ids = torch.as_tensor(np.asarray(seqs_i), dtype=torch.long)
    x = SR.zero_padded(p[TABLE])[ids] * (C ** 0.5)                                 # GRU4REC.py:35
    return stacked_gru(p, x, nb) * (ids != 0).to(x.dtype).unsqueeze(-1)            # :44-47


def gru4rec_train(p, features, labels, C, nb, l2_reg):     # (loss, training logits [B*T, I], evaluation logits [B, I])
    rows = gru4rec_rows(p, features["seqs_i"], C, nb)
    logits = SR._logits(p, TABLE, BIAS, rows.reshape(-1, C))
    return SR.all_position_loss(logits, labels) + SR._l2(p, (TABLE,), l2_reg), logits, SR._logits(p, TABLE, BIAS, rows[:, -1])
