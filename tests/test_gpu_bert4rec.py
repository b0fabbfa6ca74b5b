"""BERT4REC on the GPU: ops.BertAttnFn (edgl_battn_*) and the model against the float64 restatement of
tests/_bert4rec_ref.py.  Bounds, max-abs-error / max-abs-reference per tensor: f32 1e-4 (forward) and 1e-3 (gradients), bf16 3e-2
and 1e-1 — those of tests/test_gpu_tgrec.py / test_gpu_grec.py.  The bf16 inputs are built in bf16 and the reference gets those
rounded values."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _bert4rec_ref as BR
from tests import _seq_baselines_ref as SR
from tests._util import assert_close, rel_err, to_dev

pytestmark = pytest.mark.gpu
TOL = {torch.float32: (1e-4, 1e-3), torch.bfloat16: (3e-2, 1e-1)}


def _zero(ids, b, lo, hi):
    ids[b, lo:hi] = 0


# B, T, H, dh, the zeros of the ids: the smallest shapes at which each part can go wrong (blocks are 64 keys, tiles 16 rows)
CASES = [(1, 1, 1, 16, lambda i: None),                        # a single key
         (2, 17, 2, 16, lambda i: _zero(i, 1, 0, 17)),         # one row past a tile; sample 1 uniform over 17 keys, dV != 0
         (2, 64, 1, 32, lambda i: _zero(i, slice(None), 0, 5)),     # exactly one block
         (2, 65, 2, 64, lambda i: _zero(i, 0, 0, 64)),         # one key past a block; sample 0 skips the whole first block
         (1, 101, 2, 64, lambda i: _zero(i, 0, 50, 51)),       # the model's default length, a zero in the middle
         (1, 130, 1, 128, lambda i: _zero(i, 0, 64, 128)),     # widest head; a dead block between two live ones
         (1, 1025, 1, 16, lambda i: _zero(i, 0, 0, 700))]      # longest row; many skipped blocks


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,T,H,dh,zeros", CASES)
def test_attention_forward_and_gradient_match_float64(dtype, B, T, H, dh, zeros):
    from easydgl_amd import ops
    ftol, gtol = TOL[dtype]
    C = H * dh
    g = torch.Generator().manual_seed(B * T + C)
    qkv, d_out = torch.randn(B, T, 3 * C, generator=g).to(dtype), torch.randn(B, T, C, generator=g).to(dtype)
    ids = torch.randint(1, 50, (B, T), generator=g)
    zeros(ids)
    ref = qkv.double().requires_grad_(True)
    want = BR.bert_attention(ref, ids, H)
    want.backward(d_out.double())
    leaf = qkv.cuda().requires_grad_(True)
    out = ops.BertAttnFn.apply(leaf, ids.cuda(), H, ops.NO_DROP)
    out.backward(d_out.cuda())
    got = leaf.grad.float().cpu()
    e_out, e_grad = rel_err(out.detach().float().cpu().numpy(), want.detach().numpy()), rel_err(got.numpy(), ref.grad.numpy())
    print(f"battn {dtype} B={B} T={T} H={H} dh={dh}: out {e_out:.2e} d_qkv {e_grad:.2e}")
    assert e_out <= ftol and e_grad <= gtol
    padded = ((ids == 0) & (ids != 0).any(1, keepdim=True))[:, :, None].expand(B, T, 2 * C)
    assert (ref.grad[:, :, C:][padded] == 0).all() and (got[:, :, C:][padded] == 0).all()     # dK, dV of padded keys: exact zeros


def test_dropout_is_repeatable_shared_by_both_passes_and_unbiased():
    from easydgl_amd import ops
    B, T, H, dh, r = 4, 100, 2, 16, 0.3
    C = H * dh
    g = torch.Generator(device="cuda").manual_seed(5)
    qkv = torch.randn(B, T, 3 * C, device="cuda", generator=g).requires_grad_(True)
    d_out = torch.randn(B, T, C, device="cuda", generator=g)
    ids = torch.ones(B, T, dtype=torch.int64, device="cuda")
    drop = ops.Drop(r, ops.make_rng_state("cuda", 77), 10)
    o1 = ops.BertAttnFn.apply(qkv, ids, H, drop)
    assert torch.equal(o1, ops.BertAttnFn.apply(qkv, ids, H, drop))
    assert not torch.allclose(o1, ops.BertAttnFn.apply(qkv, ids, H, ops.NO_DROP))
    o1.backward(d_out)
    dV = torch.zeros_like(qkv)
    dV[:, :, 2 * C:] = torch.randn(B, T, C, device="cuda", generator=g)
    o2 = ops.BertAttnFn.apply((qkv + dV).detach(), ids, H, drop)
    lhs, rhs = float(((o2 - o1.detach()).double() * d_out.double()).sum()), float((qkv.grad.double() * dV.double()).sum())
    assert abs(lhs - rhs) <= 1e-3 * max(1.0, abs(rhs)), (lhs, rhs)
    flat = torch.zeros(B, T, 3 * C, device="cuda")
    flat[:, :, 2 * C:] = 1.0                       # Q = 0, V = 1: every output is (kept count) / (T (1 - r))
    mean = float(ops.BertAttnFn.apply(flat, ids, H, drop).double().mean())
    assert abs(mean - 1.0) <= 5 * (r / ((1 - r) * B * H * T * T)) ** 0.5, mean


def _flags(mode, **kw):
    base = dict(model="BERT4REC", num_items=50, num_units=32, num_heads=2, num_blocks=2, seqslen=9, masklen=2, learning_rate=1e-3,
                l2_reg=1e-3, compute_dtype=mode, num_train_steps=None, num_warmup_steps=None)
    base.update(kw)
    return SimpleNamespace(**base)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_model_loss_eval_logits_and_gradients_match_float64(mode):
    import easydgl_amd
    B, T, C, H, N, nb, l2 = 3, 10, 32, 2, 50, 2, 1e-3
    ftol, gtol = TOL[torch.float32 if mode == "f32" else torch.bfloat16]
    rng = np.random.default_rng(22)
    params = SR.init_from_shapes(BR.bert4rec_shapes(N + 2, T, C, nb), rng)
    if mode == "bf16":      # the variables are built in bf16 too: the reference gets the values the kernels read
        params = {k: torch.tensor(v).bfloat16().double().numpy() for k, v in params.items()}
    tokens = torch.tensor(rng.integers(1, N, size=(B, T)))
    tokens[0, :3] = 0
    pos = torch.tensor([[4, 8], [3, 9], [2, 7]])
    feats, labels = {"seqs_i": tokens.scatter(1, pos, N), "masked_positions": pos}, tokens.gather(1, pos)
    m = easydgl_amd.ranking(_flags(mode)).finalize("cuda")
    m.load_tf_variables(params)
    p64 = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    ref = BR.bert4rec_train_loss(p64, feats, labels, H, nb, l2)
    ref.backward()
    m.zero_grad_arena()
    loss = m.train_loss(to_dev(feats), labels.cuda())
    loss.backward()
    e_loss = abs(loss.item() - ref.item()) / abs(ref.item())
    errs = {}
    for k, g in m.tf_gradients().items():
        r = p64[k].grad.numpy()
        if k.endswith("BERTAttention/K/bias"):
            # a bias on K shifts a whole score row: its true gradient is zero, so the residue is held against the K kernel's scale
            scale_k = np.abs(p64[k.replace("bias", "kernel")].grad.numpy()).max()
            assert np.abs(r).max() < 1e-12 * scale_k
            errs[k] = float(np.abs(g).max() / scale_k)
        else:
            errs[k] = rel_err(g, r)
    print(f"bert4rec {mode}: loss err {e_loss:.2e} " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert set(errs) == set(p64) and e_loss <= ftol
    assert all(v <= gtol for v in errs.values()), {k: v for k, v in errs.items() if v > gtol}
    efeats = {"seqs_i": torch.cat([tokens[:, :-1], torch.full((B, 1), N)], 1)}
    want = BR.bert4rec_eval_logits(p64, efeats, H, nb).detach().numpy()
    with torch.no_grad():
        elog = m(to_dev(efeats), False).float().cpu().numpy()
    assert (elog[:, 0] == -1000.0).all()
    assert_close(elog[:, 1:], want[:, 1:], ftol, "eval logits")


def test_an_untiled_head_dim_is_refused_by_flag_name_before_any_launch():
    import easydgl_amd
    from easydgl_amd import ops
    qkv = torch.zeros(1, 8, 3 * 48, device="cuda")
    with pytest.raises(ValueError, match="--num_heads"):
        ops.BertAttnFn.apply(qkv, torch.ones(1, 8, dtype=torch.int64, device="cuda"), 1, ops.NO_DROP)
    with pytest.raises(ValueError, match="--num_heads"):
        easydgl_amd.ranking(_flags("bf16", num_units=96, num_heads=2))
