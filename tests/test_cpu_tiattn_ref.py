"""The float64 reference of the interval attention (tests/_tiattn_ref.py) and the inputs of tests/test_gpu_tiattn.py, checked
without a GPU: the reference equals oracle.baselines_ref.ti_attention where that can express the problem, the inputs of every GPU
case reach the buckets / paddings / clipped rows they claim, and seven deliberately wrong restatements all move a checked tensor
by at least 3 x the bound the GPU test applies to it — the condition that keeps those bounds from hiding a missing term."""
import numpy as np
import pytest
import torch

from oracle import baselines_ref as BR
from tests import _tiattn_ref as TR
from tests._util import grad_errors


def test_reference_equals_the_oracle_attention():
    """dense = dense_1 = identity, dense_2 random; key rows zero exactly where ids == 0 (the oracle masks by all-zero key rows);
    position tables of T + 3 rows; left padding, an all-padding sample, an interior pad, clipped buckets (zero-row lookups)."""
    B, T, H, dh, timelen = 3, 19, 2, 16, 12
    C = H * dh
    g = np.random.default_rng(4)
    t64 = lambda *s, k=1.0: torch.tensor(g.standard_normal(s) * k, dtype=torch.float64)
    o, kw = TR.make_inputs(B, T, H, dh, timelen, timelen, torch.float32, seed=3)
    ids = o["ids"]
    ids[1, T - 4] = 0             # with B = 3 the builder's interior pad falls into the all-padding sample: one more, in sample 1
    assert (ids[2] == 0).all() and (ids[0, :T // 3] == 0).all() and ids[0, T // 3:].all() and (ids[1] == 0).sum() == 1
    queries = t64(B, T, C)
    keys = t64(B, T, C) * (ids != 0)[..., None]
    W2, pK, pV, tK, tV = t64(C, C, k=0.2), t64(T + 3, C, k=0.3), t64(T + 3, C, k=0.3), t64(timelen, C, k=0.3), t64(timelen, C, k=0.3)
    a = "a/"
    eye, z = torch.eye(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    p = {a + "dense/kernel": eye, a + "dense/bias": z, a + "dense_1/kernel": eye, a + "dense_1/bias": z,
         a + "dense_2/kernel": W2, a + "dense_2/bias": z}
    ts32 = o["ts"].numpy() / np.float32(kw["time_scale"])                                  # oracle/baselines_ref.py:204-206
    d32 = np.clip(ts32[:, 1:, None] - ts32[:, None, :-1], np.float32(0), np.float32(timelen))
    intervals = torch.as_tensor(d32.astype(np.int64))
    assert torch.equal(intervals, torch.from_numpy(TR.buckets(o["ts"].numpy(), kw["time_scale"], timelen)))
    causal = np.tril(np.ones((T, T), dtype=bool))
    assert (d32.astype(np.int64)[:, causal] == timelen).mean() > 0.05                       # clipped buckets: zero-row lookups
    want = BR.ti_attention(p, a, queries, keys, intervals, dict(pK=pK, pV=pV, tK=tK, tV=tV), H)
    mine = dict(o, q=queries, kvp=torch.cat([keys + pK[:T], keys @ W2 + pV[:T]], -1), resid=queries, kt=tK, vt=tV)
    got = TR.reference(mine, **kw)["out"]
    err = float((got - want).abs().max())
    print(f"reference against oracle.baselines_ref.ti_attention: {err:.3e}")
    assert err <= 1e-12


def _causal_pairs(c, o, kw):
    T = c["T"]
    x = o["ts"].numpy() / np.float32(kw["time_scale"])
    raw = x[:, 1:, None] - x[:, None, :T]
    pairs = np.tril(np.ones((T, T), dtype=bool)) if kw["causal"] else np.ones((T, T), dtype=bool)
    return TR.buckets(o["ts"].numpy(), kw["time_scale"], c["timelen"])[:, pairs], raw[:, pairs]


@pytest.mark.parametrize("ci", range(len(TR.CASES)), ids=[TR.case_id(c) for c in TR.CASES])
def test_inputs_reach_what_they_claim(ci):
    """The pairs the kernel walks (q >= k under the causal flag, all pairs without) hit bucket 0, interior buckets and bucket
    `timelen`.  The one-pair case (T = 1, timelen = 1) has one bucket and no interior one: there the pair must be a valid bucket."""
    c = TR.CASES[ci]
    o, kw = TR.make_inputs(**c, seed=700 + ci)
    T, timelen, rows = c["T"], c["timelen"], c["tab_rows"]
    bk, raw = _causal_pairs(c, o, kw)
    assert bk.min() >= 0 and bk.max() <= timelen
    ids = o["ids"].numpy()
    assert (ids[0, :max(1, T // 3)] == 0).all() and (T <= 5 or ids[-1, T - 3] == 0) and (c["B"] < 3 or not ids[2].any())
    if T == 1:
        assert bk.size == 1
        return
    hit = set(np.unique(bk).tolist())
    assert 0 in hit and timelen in hit and any(0 < d < timelen for d in hit), sorted(hit)
    if rows <= timelen:
        frac = float((bk >= rows).mean())
        assert frac >= 0.05, frac
    else:
        assert rows - 1 in hit                                                    # the clipped bucket reads a real row
    if T > 8:
        assert (raw < 0).any()                                                    # a decreasing timestamp pair
    if timelen >= 15:
        assert len(hit) > 8, sorted(hit)
    if c.get("days"):
        assert np.array_equal(raw, np.rint(raw))                                  # every pair sits exactly on a bucket boundary
    if c.get("pad0"):
        assert (o["ts"].numpy()[0, :T // 3] == 0).all()
        assert (TR.buckets(o["ts"].numpy(), kw["time_scale"], timelen)[0, T - 1, :T // 3] == timelen).all()


DISCRIMINATION_CASES = [dict(B=3, T=17, H=2, dh=16, timelen=15, tab_rows=15),
                        dict(B=3, T=37, H=2, dh=64, timelen=40, tab_rows=30, epoch=True),
                        dict(B=2, T=100, H=1, dh=32, timelen=256, tab_rows=256, epoch=True)]


@pytest.mark.parametrize("ci", range(len(DISCRIMINATION_CASES)), ids=[TR.case_id(c) for c in DISCRIMINATION_CASES])
def test_wrong_forms_move_a_checked_tensor_by_three_bounds(ci):
    """bf16-rounded operands and the bf16 bounds (the wider ones): every wrong form differs from the true reference by >= 3 x the
    bound of the GPU test in at least one tensor it checks, in the norm that bound applies to."""
    c = DISCRIMINATION_CASES[ci]
    o, kw = TR.make_inputs(**c, dtype=torch.bfloat16, seed=900 + ci)
    true = TR.reference(o, **kw)
    tol = {k: np.maximum(TR.bounds("bf16")[k], TR.bounds("f32")[k]) for k in TR.FORWARD + TR.GRADS}
    for form in TR.WRONG_FORMS:
        bad = TR.reference(o, **kw, wrong=form)
        moved = {}
        for k in ("out",) + TR.GRADS:
            l2, mx = grad_errors(bad[k].numpy(), true[k].numpy())
            moved[k] = (l2 / tol[k][0], mx / tol[k][1])
        print(form, {k: f"{v[0]:.1f}x / {v[1]:.1f}x" for k, v in moved.items()})
        assert max(max(v) for v in moved.values()) >= 3.0, (form, moved)
