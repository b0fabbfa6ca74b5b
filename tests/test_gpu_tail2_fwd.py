"""The forward of the two-per-CU block tail (csrc/k_tail_fwd.hip, t2::tail2_fwd_kernel) stores through a uniform base + 32-bit lane
offsets that every store batch rebuilds (copy_out, gelu_pass, the lane's operand offsets behind each batch) — the form that keeps
the kernel free of scratch (DESIGN rule 80).  Same addresses, same bytes: every tensor the forward writes, pre-filled with NaN, must
come out bit for bit as from the one-per-CU kernel with no NaN left (the gathered head rows: no row left zero), at the sizes where
offsets and guards differ: one sample and several (the uniform base moves by T rows), T = 2 / 17 / 50 / 101 (the three row-tile
instantiations; one row in a second tile; every row of the largest image), a head gather of 1 and of 20 rows per sample (less and
more than one round of 512 threads / 16)."""
import pytest
import torch

from tests._util import build_model, make_problem, to_dev

pytestmark = pytest.mark.gpu

FWD_BLOCK = ("ao", "a1", "pre_f", "f", "o", "y", "st1", "st2")
FWD_HEAD = ("pre_t", "so", "st3")


def _forward(prob, batch, variant):
    from easydgl_amd import _lib
    from easydgl_amd.engine import TrainEngine
    prev = _lib.lib.edgl_tail_variant(variant)
    try:
        m = build_model(prob, "bf16", hidden_drop=0.1, att_drop=0.1)
        eng = TrainEngine(m, batch, use_graph=False)
        assert eng.fused_tail
        eng.load_batch(to_dev(prob["feats"]), torch.as_tensor(prob["labels"]).cuda())
        for b in eng.blk:
            for k in FWD_BLOCK:
                b[k].fill_(float("nan"))
        for k in FWD_HEAD:
            getattr(eng, k).fill_(float("nan"))
        # (hrows_c stays as the engine prepared it, zero-filled: the scoring's matrix instructions read the rows behind the weighted ones)
        eng._issue()
        torch.cuda.synchronize()
        out = {k: getattr(eng, k).clone() for k in FWD_HEAD}
        out["hrows"] = eng.hrows_c[:int(eng.nvalid[0])].clone()
        out["loss"] = eng.loss.clone()
        for i, b in enumerate(eng.blk):
            for k in FWD_BLOCK:
                out[f"{k}{i}"] = b[k].clone()
        return out
    finally:
        _lib.lib.edgl_tail_variant(prev)


def _problem(batch, seqslen, masklen):
    """The first seed whose batch has a weighted (label != 0) masked slot: without one the loss of either kernel is 0 / 0."""
    import numpy as np
    for seed in range(31 + seqslen + masklen, 131 + seqslen + masklen):
        prob = make_problem(seed=seed, batch=batch, num_units=128, num_heads=8, num_blocks=2, seqslen=seqslen, masklen=masklen,
                            num_events=16, num_items=300)
        if int((np.asarray(prob["labels"]) != 0).sum()) > 0:
            return prob
    raise AssertionError("no seed with a weighted slot")


@pytest.mark.parametrize("seqslen,masklen", [(1, 1), (16, 1), (16, 3), (49, 9), (100, 1), (100, 20)])
@pytest.mark.parametrize("batch", [1, 3])
def test_forward_outputs_are_those_of_the_one_per_cu_kernel(batch, seqslen, masklen):
    prob = _problem(batch, seqslen, masklen)
    one, two = _forward(prob, batch, 0), _forward(prob, batch, 1)
    assert set(one) == set(two)
    for k in two:
        for out in (one, two):
            assert not bool(torch.isnan(out[k].float()).any()), ("NaN left in", k)
        if k == "hrows":
            assert bool((two[k].float().abs().amax(dim=1) > 0).all()), "a gathered row was not written"
        if k == "loss":
            assert abs(float(one[k]) - float(two[k])) <= 1e-6 * abs(float(one[k]))
        else:
            assert torch.equal(one[k], two[k]), (k, float((one[k].float() - two[k].float()).abs().max()))
