"""The additive-attention kernel pair (csrc/k_addattn.hip) through ops.AddAttnFn against the float64 expression of its
definition: out, d_a12, d_h, d_v at one position, one key past a tile, a width that is no power of two, several tiles and the
widest rows; left padding of a different length per sample, a zero id inside a sequence, an all-padding sample.  Bounds: the
small-case bounds of tests/_util.py (GRAD_TOL: f32 1e-3, bf16 rel-L2 2e-2 / max 5e-2) on every output.  bf16: the reference reads
the bf16-rounded inputs."""
import pytest
import torch

from tests._util import GRAD_TOL, grad_errors

pytestmark = pytest.mark.gpu
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def _inputs(B, T, C, dtype, all_padding=False):
    g = torch.Generator().manual_seed(1000 * B + 10 * T + C)
    h, a12, d_out = (torch.randn(B, T, w, generator=g).to(dtype) for w in (C, 2 * C, C))
    v = torch.randn(C, generator=g) / C ** 0.5
    ids = torch.randint(1, 50, (B, T), generator=g)
    for b in range(B):
        ids[b, :(3 * b + 2) % T] = 0              # left padding, another length per sample
    if T >= 4:
        ids[0, T - 2] = 0                         # a zero inside a sequence
    if B >= 2 or all_padding:
        ids[0 if all_padding else B - 1:] = 0     # a sample (or all of them) without a real key
    return h, a12, v, ids, d_out


def _reference(h, a12, v, ids, d_out):
    h, a12, v, d_out = (x.double().requires_grad_(x is not d_out) for x in (h, a12, v, d_out))
    T, C = h.shape[1], h.shape[2]
    e = (torch.sigmoid(a12[:, :, None, :C] + a12[:, None, :, C:]) * v).sum(-1)                  # [B, T(t), T(j)]
    mask = torch.tril(torch.ones(T, T, dtype=torch.bool)) & (ids != 0)[:, None, :]
    out = (e * mask) @ h
    out.backward(d_out)
    return out.detach(), a12.grad, h.grad, v.grad


def _run(h, a12, v, ids, d_out):
    from easydgl_amd import ops
    h, a12, v = (x.cuda().requires_grad_() for x in (h, a12, v))
    out = ops.AddAttnFn.apply(h, a12, v, ids.cuda())
    out.backward(d_out.cuda())
    return [x.detach().float().cpu() for x in (out, a12.grad, h.grad, v.grad)]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("B,T,C", [(2, 1, 32), (3, 17, 32), (2, 16, 48), (2, 40, 128), (1, 33, 512)])
def test_forward_and_backward_match_float64(B, T, C, mode):
    args = _inputs(B, T, C, DTYPES[mode])
    got, want = _run(*args), _reference(*args)
    errs = {n: grad_errors(g.numpy(), w.numpy()) for n, g, w in zip(("out", "d_a12", "d_h", "d_v"), got, want)}
    print(f"addattn {mode} B={B} T={T} C={C}: (rel-L2, max) {errs}")
    assert all(l2 <= GRAD_TOL[mode][0] and mx <= GRAD_TOL[mode][1] for l2, mx in errs.values()), errs
    if B >= 2:                                    # the all-padding sample: exact zeros in everything it owns
        assert all(not x[B - 1].any() for x in got[:3])


def test_all_padding_gives_exact_zeros():
    got = _run(*_inputs(2, 17, 32, torch.bfloat16, all_padding=True))
    assert all(not x.any() for x in got)


def test_backward_twice_gives_the_same_bits():
    args = _inputs(3, 40, 128, torch.bfloat16)
    first, second = _run(*args), _run(*args)
    assert all(torch.equal(a, b) for a, b in zip(first[1:], second[1:]))
