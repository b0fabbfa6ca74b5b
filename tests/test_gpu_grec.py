"""GREC on the GPU: ops.DConvLnFn (edgl_dconv_ln_*) and the model against the float64 restatement of
tests/_grec_ref.py (shift-and-matmul, no conv call).  Bounds, max-abs-error / max-abs-reference per tensor: f32 1e-4 (forward) and
1e-3 (gradients), bf16 3e-2 and 1e-1 — those of tests/test_gpu_tgrec.py.  The bf16 inputs are built in bf16 and the reference
gets those rounded values."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _grec_ref as GR
from tests import _seq_baselines_ref as SR
from tests._util import assert_close, rel_err, to_dev

pytestmark = pytest.mark.gpu
TOL = {torch.float32: (1e-4, 1e-3), torch.bfloat16: (3e-2, 1e-1)}
BOTH = (False, True)
# B, T, C, fw, d, causal forms, residual: the smallest shapes at which each part can go wrong (the row block is 64 rows)
CASES = [(1, 1, 32, 3, 1, BOTH, False),       # every tap but one out of range
         (2, 5, 32, 3, 4, BOTH, True),        # reach longer than the sequence
         (2, 17, 128, 3, 1, (True,), True),   # one row past a 16-row tile
         (2, 16, 32, 2, 3, (False,), False),  # even width: asymmetric SAME padding, left 1, right 2
         (3, 65, 128, 3, 8, BOTH, True),      # halo crossing a row-block edge, reach above one tile
         (1, 130, 64, 5, 2, (False,), False), # widest filter, three row blocks
         (2, 33, 512, 3, 2, (True,), True)]   # widest row, four column blocks of the weight gradient
OP_CASES = [(B, T, C, fw, d, c, res) for B, T, C, fw, d, cs, res in CASES for c in cs]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,T,C,fw,d,causal,residual", OP_CASES)
def test_dconv_ln_forward_and_every_gradient_match_float64(dtype, B, T, C, fw, d, causal, residual):
    from easydgl_amd import ops
    ftol, gtol = TOL[dtype]
    rng = np.random.default_rng(B * T + C + fw + d)
    mk = lambda *s, sc=1.0, add=0.0: (torch.tensor(rng.standard_normal(s), dtype=torch.float32) * sc + add)
    x, r, dy, w = mk(B, T, C).to(dtype), mk(B, T, C).to(dtype), mk(B, T, C).to(dtype), mk(fw, C, C, sc=(fw * C) ** -0.5).to(dtype)
    bias, gamma, beta = mk(C, sc=0.1), mk(C, sc=0.1, add=1.0), mk(C, sc=0.1)
    names = ("x", "w", "bias", "gamma", "beta") + (("r",) if residual else ())
    src = (x, w, bias, gamma, beta) + ((r,) if residual else ())
    ref = [t.double().requires_grad_(True) for t in src]
    want = GR.dconv_ln(*ref[:5], d, causal, ref[5] if residual else None)
    want.backward(dy.double())
    # the f32 master of w is the gradient's leaf, its activation-dtype copy what the kernels read
    leaves = [t.float().cuda().requires_grad_(True) if n == "w" else t.cuda().requires_grad_(True) for n, t in zip(names, src)]
    out = ops.DConvLnFn.apply(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], w.cuda(), d, causal, leaves[5] if residual else None)
    out.backward(dy.cuda())
    errs = {"y": rel_err(out.detach().float().cpu().numpy(), want.detach().numpy())}
    for n, got, rf in zip(names, leaves, ref):
        errs["d" + n] = rel_err(got.grad.float().cpu().numpy(), rf.grad.numpy())
    print(f"dconv {dtype} B={B} T={T} C={C} fw={fw} d={d} causal={causal}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs.pop("y") <= ftol
    assert all(v <= gtol for v in errs.values()), errs


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_model_loss_eval_logits_and_gradients_match_float64(mode):
    import easydgl_amd
    from easydgl_amd import data as D
    B, T, C, N, fw, dil = 3, 10, 32, 50, 3, [1, 2]
    ftol, gtol = TOL[torch.float32 if mode == "f32" else torch.bfloat16]
    rng = np.random.default_rng(21)
    params = SR.init_from_shapes(GR.grec_shapes(N + 2, C, fw, dil), rng)
    for k, v in params.items():
        if v.ndim == 3:
            params[k] = (rng.standard_normal(v.shape) * (fw * C) ** -0.5).astype(np.float32).astype(np.float64)
    if mode == "bf16":      # the variables are built in bf16 too: the reference gets the values the kernels read
        params = {k: torch.tensor(v).bfloat16().double().numpy() for k, v in params.items()}
    tokens = torch.tensor(rng.integers(1, N, size=(B, T)))
    tokens[0, :3] = 0                                                   # left padding: id 0 is embedded, the label 0 carries no weight
    feats, labels = D.grec_mask_random(tokens, N, torch.tensor([[1, 5], [3, 9], [2, 7]]))
    F = SimpleNamespace(model="GREC", num_items=N, num_units=C, num_heads=1, num_blocks=1, seqslen=T - 1, masklen=2, filter_width=fw,
                        dilations="1,2", learning_rate=1e-3, l2_reg=0.0, compute_dtype=mode, num_train_steps=None, num_warmup_steps=None)
    m = easydgl_amd.ranking(F).finalize("cuda")
    m.load_tf_variables(params)
    p64 = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    ref = GR.grec_train_loss(p64, feats, labels, dil)
    ref.backward()
    m.zero_grad_arena()
    loss = m.train_loss(to_dev(feats), labels.cuda())
    loss.backward()
    e_loss = abs(loss.item() - ref.item()) / abs(ref.item())
    errs = {k: rel_err(g, p64[k].grad.numpy()) for k, g in m.tf_gradients().items()}
    print(f"grec {mode}: loss err {e_loss:.2e} " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert set(errs) == set(p64) and e_loss <= ftol
    assert all(v <= gtol for v in errs.values()), {k: v for k, v in errs.items() if v > gtol}
    efeats = {"seqs_i": tokens[:, :-1].contiguous()}
    want = GR.grec_eval_logits(p64, efeats, dil).detach().numpy()
    with torch.no_grad():
        elog = m(to_dev(efeats), False).float().cpu().numpy()
    assert (elog[:, 0] == -1000.0).all() and (elog[:, -1] == -1000.0).all()
    assert_close(elog[:, 1:-1], want[:, 1:-1], ftol, "eval logits")


def test_a_halo_the_lds_cannot_hold_is_refused_by_flag_name():
    """(fw - 1) d above edgl_dconv_max_reach raises before any launch: from the op and from the model's constructor."""
    import easydgl_amd
    from easydgl_amd import _lib, ops
    C = 512
    most = _lib.lib.edgl_dconv_max_reach(C, _lib.BF16)
    assert 32 <= most < 1024                                            # (the published recipe's reach fits, the bound is real)
    x = torch.zeros(1, 8, C, device="cuda", dtype=torch.bfloat16)
    w, v = torch.zeros(3, C, C, device="cuda", dtype=torch.bfloat16), torch.zeros(C, device="cuda")
    with pytest.raises(ValueError, match="--dilations"):
        ops.DConvLnFn.apply(x, w.float(), v, v, v, w, most // 2 + 1, True, None)
    F = SimpleNamespace(model="GREC", num_items=50, num_units=C, num_heads=1, seqslen=9, masklen=2, filter_width=3,
                        dilations=f"1,{most // 4 + 1}", learning_rate=1e-3, compute_dtype="bf16")
    with pytest.raises(ValueError, match="--dilations"):
        easydgl_amd.ranking(F)
