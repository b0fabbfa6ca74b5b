"""TGREC on the GPU: ops.TgAttnFn (edgl_tgattn_* + its per-head GEMMs) and the model against the float64 restatement
of tests/_tgrec_ref.py, which materialises Phi(dt) with the clamp.  Bounds, max-abs-error / max-abs-reference per tensor: f32 1e-4
(forward) and 1e-3 (gradients), bf16 3e-2 and 1e-1 — those of tests/test_gpu_tgat.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _seq_baselines_ref as SR
from tests import _tgrec_ref as TG
from tests._util import assert_close, rel_err, to_dev

pytestmark = pytest.mark.gpu
TOL = {torch.float32: (1e-4, 1e-3), torch.bfloat16: (3e-2, 1e-1)}


def _padding_and_times(rng, B, T):
    """ids with a left pad ending mid-tile, a padded key away from the edge and an all-padding sequence; sorted times, zeros under
    the left padding (tests/test_gpu_tgat.py _operands)."""
    ids = torch.tensor(rng.integers(1, 50, size=(B, T)))
    ids[0, :max(1, T // 3)] = 0
    if T > 5:
        ids[-1, T - 3] = 0
    if B >= 3:
        ids[2, :] = 0
    real = (torch.cumsum(ids != 0, 1) > 0).double()
    t = torch.cumsum(torch.tensor(rng.uniform(0.0, 0.25, size=(B, T))) * real, 1)
    return ids, t


def _operands(seed, B, T, H, C, dtype):
    rng = np.random.default_rng(seed)
    mk = lambda *s, sc=1.0: (torch.tensor(rng.standard_normal(s), dtype=torch.float32) * sc).to(dtype)
    q, kv, d_out, w = mk(B, T, C), mk(B, T, 2 * C), mk(B, T, C), mk(2 * C, 2 * C, sc=(2 * C) ** -0.5)
    omega = torch.tensor(np.linspace(0, 9, C) + 0.1 * rng.standard_normal(C), dtype=torch.float32)
    phi = torch.tensor(0.5 * rng.standard_normal(C), dtype=torch.float32)
    ids, t = _padding_and_times(rng, B, T)
    return q, kv, w, omega, phi, d_out, ids, t.float()


def _run(q, kv, w, omega, phi, ids, t, H, drop=None):
    from easydgl_amd import ops
    leaves = [x.detach().clone().requires_grad_(True) for x in (q, kv, w.float(), omega, phi)]
    out = ops.TgAttnFn.apply(leaves[0], leaves[1], leaves[2], w, leaves[3], leaves[4], ids, t, H, 1.0, drop or ops.NO_DROP)
    return out, leaves


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,T,H,C", [(1, 1, 1, 32), (2, 16, 2, 32), (2, 17, 1, 128), (3, 33, 8, 128), (2, 40, 2, 64)])
def test_tgattn_forward_and_every_gradient_match_float64(dtype, B, T, H, C):
    ftol, gtol = TOL[dtype]
    q, kv, w, omega, phi, d_out, ids, t = _operands(B * T + C + H, B, T, H, C, dtype)
    ref = [x.double().requires_grad_(True) for x in (q, kv, w, omega, phi)]
    want = TG.tg_core(ref[0], ref[1], ref[2][C:], ref[3], ref[4], ids, t.double(), H)
    want.backward(d_out.double())
    out, leaves = _run(*[x.cuda() for x in (q, kv, w, omega, phi, ids, t)], H)
    out.backward(d_out.cuda())
    errs = {"out": rel_err(out.detach().float().cpu().numpy(), want.detach().numpy())}
    for name, got, r in zip(("d_q", "d_kv", "d_w", "d_omega", "d_phi"), leaves, ref):
        g, rg = got.grad.float().cpu().numpy(), r.grad.numpy()
        if name == "d_w":       # the op owns the time-half rows (the U path and the G path); the x half belongs to the dense op
            assert not g[:C].any()
            g, rg = g[C:], rg[C:]
        errs[name] = rel_err(g, rg)
    print(f"tgattn {dtype} B={B} T={T} H={H} C={C}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs.pop("out") <= ftol
    assert all(v <= gtol for v in errs.values()), errs


def test_tgattn_dropout_uses_one_mask_forward_and_backward():
    """With dropout the output is linear in the value half of kv for a fixed mask: <d_out, out(v + dv) - out(v)> = <d_v, dv>."""
    from easydgl_amd import ops
    B, T, H, C = 2, 40, 2, 64
    q, kv, w, omega, phi, d_out, ids, t = [x.cuda() for x in _operands(5, B, T, H, C, torch.float32)]
    drop = ops.Drop(0.3, torch.tensor([1234, 5], dtype=torch.int64, device="cuda"), 7)
    out, leaves = _run(q, kv, w, omega, phi, ids, t, H, drop)
    out.backward(d_out)
    assert not torch.allclose(out, _run(q, kv, w, omega, phi, ids, t, H)[0])
    dv = torch.randn(B, T, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    kv2 = kv.clone()
    kv2[:, :, C:] += dv
    out2 = _run(q, kv2, w, omega, phi, ids, t, H, drop)[0]
    lhs, rhs = float(((out2 - out).detach() * d_out).sum()), float((leaves[1].grad[:, :, C:] * dv).sum())
    assert abs(lhs - rhs) <= 1e-3 * max(1.0, abs(rhs)), (lhs, rhs)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_model_loss_eval_logits_and_gradients_match_float64(mode):
    import easydgl_amd
    B, T, C, H, I, nb, scale = 3, 9, 32, 2, 50, 2, 3600.0
    ftol, gtol = TOL[torch.float32 if mode == "f32" else torch.bfloat16]
    rng = np.random.default_rng(11)
    params = SR.init_from_shapes(TG.tgrec_shapes(I, T, C, nb), rng)
    params["TGREC/tcoding/basis_freq"] = (np.linspace(0, 9, C) + params["TGREC/tcoding/basis_freq"]).astype(np.float32).astype(np.float64)
    ids, t = _padding_and_times(rng, B, T)
    labels = torch.tensor(rng.integers(1, I, size=(B, T)))          # the padded positions carry real labels too (Base.py:119-140)
    ts = torch.cat([t, t[:, -1:] + 0.1], 1).float() * scale           # [B, T+1] as the reader emits it: the first T are used
    feats = {"seqs_i": ids.numpy(), "seqs_t": ts.numpy()}
    F = SimpleNamespace(model="TGREC", num_items=I, num_units=C, num_heads=H, num_blocks=nb, seqslen=T, learning_rate=1e-3, l2_reg=1e-3,
                        hidden_dropout_rate=0.0, attention_probs_dropout_rate=0.0, compute_dtype=mode, num_train_steps=None,
                        num_warmup_steps=None, time_scale=scale)
    m = easydgl_amd.ranking(F).finalize("cuda")
    m.load_tf_variables(params)
    p64 = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    ref = TG.tgrec_train_loss(p64, feats, labels.numpy(), C, H, nb, scale, 1e-3)
    ref.backward()
    dev = to_dev(feats)
    m.zero_grad_arena()
    loss = m.train_loss(dev, labels.cuda())
    loss.backward()
    m.check_inputs()
    e_loss = abs(loss.item() - ref.item()) / abs(ref.item())
    errs = {}
    for k, g in m.tf_gradients().items():
        r = p64[k].grad.numpy()
        if k.endswith("dense_1/bias") and "attention" in k:
            # a bias on K shifts a whole score row: its true gradient is zero, so the residue is held against the K kernel's scale
            scale_k = np.abs(p64[k.replace("bias", "kernel")].grad.numpy()).max()
            assert np.abs(r).max() < 1e-12 * scale_k
            errs[k] = float(np.abs(g).max() / scale_k)
        else:
            errs[k] = rel_err(g, r)
    print(f"tgrec {mode}: loss err {e_loss:.2e} " + " ".join(f"{k.split('/', 1)[-1]} {v:.2e}" for k, v in errs.items()))
    assert set(errs) == set(p64) and e_loss <= ftol
    assert all(v <= gtol for v in errs.values()), {k: v for k, v in errs.items() if v > gtol}
    want = TG.tgrec_eval_logits(p64, feats, C, H, nb, scale).detach().numpy()
    with torch.no_grad():
        elog = m(dev, False)
        assert_close(elog.float().cpu().numpy()[:, 1:], want[:, 1:], ftol, "eval logits")
        # the [B, T] form is taken as is, and a time below its predecessor is counted
        assert torch.equal(m({**dev, "seqs_t": dev["seqs_t"][:, :T].contiguous()}, False), elog)
        bad = dev["seqs_t"].clone()
        bad[1, 4] = bad[1, 3] - 1.0
        m({**dev, "seqs_t": bad}, False)
    with pytest.raises(ValueError, match="decreasing"):
        m.check_inputs()
