"""float64 torch restatement of NARM: scaled zero-padded item embedding, torch.nn.GRU(num_layers=L) loaded from the
model's own variables, the dense expression of the additive attention (no softmax, keys j <= t with id != 0), [h | c_local] through the
bias-free decoder, row mask, tied scoring, cross-entropy, l2 of the table."""
import numpy as np
import torch

from tests import _seq_baselines_ref as SR

GRU_SCOPE = "NARM/GRU/opaque_kernel/"
TABLE, BIAS = "NARM/item_embs/lookup_table", "NARM/output_bias"
A1, A2, V, DEC = "NARM/attention/A1/kernel", "NARM/attention/A2/kernel", "NARM/attention/v", "NARM/decoder/kernel"
_PARTS = (("weight_ih", "w_"), ("bias_ih", "b_w"), ("weight_hh", "r_"), ("bias_hh", "b_r"))


def narm_shapes(I, C, nb):
    s = {TABLE: (I, C), BIAS: (I - 1,), A1: (C, C), A2: (C, C), V: (C,), DEC: (2 * C, C)}
    for l in range(nb):
        for g in SR.GRU_GATES:      # weights in tf.layers.dense orientation [in, out]
            s[GRU_SCOPE + f"{l}/w_{g}"] = s[GRU_SCOPE + f"{l}/r_{g}"] = (C, C)
            s[GRU_SCOPE + f"{l}/b_w{g}"] = s[GRU_SCOPE + f"{l}/b_r{g}"] = (C,)
    return s


def narm_params(I, C, nb, rng):
    p = SR.init_from_shapes(narm_shapes(I, C, nb), rng)
    p[V] = SR.glorot(rng, (C, 1)).reshape(C).astype(np.float32).astype(np.float64)      # (a vector, but glorot like the model's)
    return p


def narm_train(params, features, labels, C, nb, l2_reg):
    """(loss, training logits [B*T, I], evaluation logits [B, I], {variable name: gradient})."""
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items() if not k.startswith(GRU_SCOPE)}
    gru = torch.nn.GRU(C, C, num_layers=nb, batch_first=True).double()
    with torch.no_grad():           # torch keeps [3C, in] blocks in the order r | z | n: the [in, out] parts transposed
        for l in range(nb):
            for name, pre in _PARTS:
                v = torch.cat([torch.as_tensor(params[GRU_SCOPE + f"{l}/{pre}{g}"]) for g in SR.GRU_GATES], dim=-1)
                getattr(gru, f"{name}_l{l}").copy_(v.t() if v.dim() == 2 else v)
    ids = torch.as_tensor(np.asarray(features["seqs_i"]), dtype=torch.long)
    T = ids.shape[1]
    h = gru(SR.zero_padded(p[TABLE])[ids] * (C ** 0.5))[0]
    e = (torch.sigmoid((h @ p[A1])[:, :, None, :] + (h @ p[A2])[:, None, :, :]) * p[V]).sum(-1)
    alpha = e * (torch.tril(torch.ones(T, T, dtype=torch.bool)) & (ids != 0)[:, None, :])
    rows = (torch.cat([h, alpha @ h], dim=-1) @ p[DEC]) * (ids != 0).to(h.dtype).unsqueeze(-1)
    logits = SR._logits(p, TABLE, BIAS, rows.reshape(-1, C))
    loss = SR.all_position_loss(logits, labels) + SR._l2(p, (TABLE,), l2_reg)
    loss.backward()
    grads = {k: v.grad.numpy() for k, v in p.items()}
    for l in range(nb):
        for name, pre in _PARTS:
            g = getattr(gru, f"{name}_l{l}").grad
            g = g.t() if g.dim() == 2 else g
            for j, gate in enumerate(SR.GRU_GATES):
                grads[GRU_SCOPE + f"{l}/{pre}{gate}"] = g[..., j * C:(j + 1) * C].numpy()
    return loss.item(), logits.detach().numpy(), SR._logits(p, TABLE, BIAS, rows[:, -1]).detach().numpy(), grads
