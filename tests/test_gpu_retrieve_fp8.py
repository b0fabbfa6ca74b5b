"""FP8 two-stage retrieval on the GPU: the quantiser against the e4m3 format, stage 1 against float64 on the kernel's
own bytes, the two-stage result against today's exact top-K when the short list covers the catalogue, and the driver's metrics."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests._util import build_model, make_problem, to_dev

pytestmark = pytest.mark.gpu
FWD_TOL = 1e-4      # the f32 forward bound of the parity tests: max-abs error / max-abs reference


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("R,C", [(1, 32), (33, 128), (5, 512)])
def test_quantiser_is_within_half_an_e4m3_step(R, C, dtype):
    from easydgl_amd import ops
    g = torch.Generator().manual_seed(R * C)
    x = torch.randn(R, C, generator=g)
    if R >= 5:
        x[1] = 0.0                  # a zero row: scale 1
        x[2, 3] = 1e30              # one huge element: everything else rounds to zero
        x[3] *= 1e-30               # a tiny scale
        x[4, ::2] *= 1e-4           # quotients below e4m3's smallest normal
    x = x.to(dtype).cuda()
    q8, scale = ops.rows_to_fp8(x)
    xf = x.float().cpu()
    mx = xf.abs().amax(1)
    want = torch.where(mx > 0, mx / 448.0, torch.ones_like(mx))
    assert torch.allclose(scale.cpu(), want, rtol=2.0 ** -23, atol=0.0)
    y = xf.double() / scale.cpu().double()[:, None]
    deq = q8.cpu().view(torch.float8_e4m3fn).double()
    binade = torch.exp2(torch.frexp(y.abs().clamp_min(2.0 ** -6))[1].double() - 1.0)
    half_step = torch.where(y.abs() >= 2.0 ** -6, binade * 2.0 ** -4, torch.full_like(y, 2.0 ** -10))
    # (the kernel divides in f32: a quotient may sit 2^-24 off the float64 one, which matters only at a rounding midpoint)
    assert bool(((deq - y).abs() <= half_step * (1 + 1e-6)).all()), float(((deq - y).abs() / half_step).max())


def _chunk():
    from easydgl_amd import ops
    return ops.FP8_CHUNK_ITEMS


@pytest.mark.parametrize("R,C,I,i0,K,T,copies", [(1, 32, 4104, 8, 1, 0, 0), (33, 128, 4099 + 8, 8, 50, 7, 0), (130, 512, 9000, 0, 128, 7, 0),
                                                 (3, 256, 5000, 0, 1024, 3, 0), (2, 32, None, 0, 20, 3, 0), (3, 64, 64 * 70, 0, 40, 5, 64)])
def test_stage1_against_float64_on_the_same_bytes(R, C, I, i0, K, T, copies):
    from easydgl_amd import ops
    I = _chunk() + 5000 if I is None else I          # two chunks and the merge
    g = torch.Generator().manual_seed(C + K)
    rows, table, bias = torch.randn(R, C, generator=g), torch.randn(I, C, generator=g), 0.1 * torch.randn(I - 1, generator=g)
    if copies:                                       # one row, copied: the id tie rule decides alone and every list overflows
        table, bias = table[:1].repeat(I, 1), torch.zeros(I - 1)
    table[0] = 0.0
    seen = None
    if T:
        seen = torch.randint(0, I, (R, T), generator=g)
        seen[:, 0], seen[:, 1] = 0, seen[:, 2]       # zeros and duplicates
    rq, rs = ops.rows_to_fp8(rows.cuda())
    tq, ts = ops.rows_to_fp8(table.cuda())
    val, idx = ops.score_topk_fp8(rq, rs, tq, ts, bias.cuda(), None if seen is None else seen.cuda(), K, i0, I)
    val, idx = val.cpu().double(), idx.cpu().long()

    def deq(q, s):
        return q.cpu().view(torch.float8_e4m3fn).double() * s.cpu().double()[:, None]
    ref = deq(rq, rs) @ deq(tq, ts).T + torch.cat([torch.tensor([-1000.0]), bias]).double()
    ref[:, 0] = -1000.0
    tol = FWD_TOL * float(ref[:, 1:].abs().max())
    if seen is not None:
        ref.scatter_(1, seen, float("-inf"))
    ref[:, :i0] = float("-inf")
    order = torch.sort(-ref, dim=1, stable=True)[1][:, :K]       # (value desc, id asc)
    for r in range(R):
        ids = idx[r]
        assert ids.unique().numel() == K and bool((ids >= max(i0, 1)).all()) and bool((ids < I).all())
        assert seen is None or not bool(torch.isin(ids, seen[r]).any())
        dv = val[r, 1:] - val[r, :-1]
        assert bool((dv <= 0).all()) and bool((ids[1:] > ids[:-1])[dv == 0].all())
        assert float((val[r] - ref[r, ids]).abs().max()) <= tol
        assert float(ref[r, order[r, -1]]) <= float(val[r, -1]) + tol        # no better item was dropped
        if copies:
            assert torch.equal(ids, order[r])


def _seq_model(kind, mode, C, I=50, T=45):
    import easydgl_amd
    from tests import _seq_baselines_ref as SR
    rng = np.random.default_rng(11)
    params = SR.init_from_shapes(SR.sasrec_shapes(I, T, C, 2), rng)
    F = SimpleNamespace(model=kind, num_items=I, num_units=C, num_heads=2, num_blocks=2, seqslen=T, learning_rate=1e-3, l2_reg=1e-3,
                        hidden_dropout_rate=0.0, attention_probs_dropout_rate=0.0, compute_dtype=mode, num_train_steps=None,
                        num_warmup_steps=None)
    m = easydgl_amd.ranking(F).finalize("cuda")
    m.load_tf_variables(params)
    return m, to_dev({"seqs_i": rng.integers(1, I, size=(6, T)), "seqs_t": np.zeros((6, T + 1), dtype=np.float32)})


@pytest.mark.parametrize("kind,mode,C", [("EasyDGL", "f32", 32), ("EasyDGL", "bf16", 64), ("SASREC", "f32", 64), ("SASREC", "bf16", 32)])
def test_covering_short_list_gives_the_exact_topk(kind, mode, C):
    from easydgl_amd import ops
    if kind == "EasyDGL":
        prob = make_problem(seed=5, batch=6, num_items=50, seqslen=45, num_units=C, num_heads=2, num_blocks=1)
        m, feats = build_model(prob, mode), to_dev(prob["efeats"])
    else:
        m, feats = _seq_model(kind, mode, C)
    n_seen = getattr(m, "mask", m.num_items) - 10                      # a row that has seen every item but K (9 real ids and item 0)
    feats["seqs_i"][3, :-1 if kind == "EasyDGL" else None] = 1         # (EasyDGL's last position holds the MASK id)
    feats["seqs_i"][3, :n_seen] = torch.arange(1, n_seen + 1, device="cuda")
    with pytest.raises(RuntimeError, match="quantize_items"):
        m.retrieve(feats, K=10)
    m.quantize_items()
    val, idx = m.retrieve(feats, K=10, shortlist=m.num_items)
    rows = m._last_rows(feats)
    wval, widx = ops.score_topk(rows, m.compute(m.item_embs.lookup_table), m.output_bias, feats["seqs_i"], 10, 0, m.num_items)
    bad = (idx != widx).any(1).nonzero().flatten().tolist()
    assert not bad, [(r, idx[r, -3:].tolist(), widx[r, -3:].tolist(), val[r, -3:].tolist(), wval[r, -3:].tolist()) for r in bad]
    assert float((val - wval).abs().max()) <= FWD_TOL * float(wval[wval > -999.0].abs().max())      # (-1000: the padding item)


def test_driver_metrics_with_a_covering_short_list_equal_the_plain_path():
    from easydgl_amd import train
    prob = make_problem(seed=6, batch=20, num_items=300, seqslen=20, num_units=32, num_heads=2, num_blocks=1)
    m = build_model(prob, "f32")
    ids, ts = np.asarray(prob["ids"]), np.asarray(prob["ts"], dtype=np.float32)
    base = train.evaluate(m, ids, ts, 8, True)
    got = train.evaluate(m, ids, ts, 8, True, fp8_shortlist=m.num_items)
    assert tuple(got) == tuple(base) and all(abs(got[k] - base[k]) <= 1e-6 * max(base[k], 1e-30) for k in base), (got, base)


def test_driver_flag_reaches_retrieve(tmp_path, monkeypatch):
    from easydgl_amd import data as D
    from easydgl_amd import formats as F
    from easydgl_amd import train as TR
    from easydgl_amd.model.base import Sequential
    ids, ts = D.synthetic_batch(300, 20, 120, seed=3)
    for name, lo, hi in (("train", 0, 80), ("valid", 80, 100), ("test", 100, 120)):
        F.write_tfrecord(str(tmp_path / f"{name}.tfrec"), [F.encode_example({"seqs_i": ids[i], "seqs_t": ts[i]}) for i in range(lo, hi)])
    calls, plain = [], Sequential.retrieve
    monkeypatch.setattr(Sequential, "retrieve", lambda self, f, K, shortlist=None, mask_seen=True: (
        calls.append(shortlist), plain(self, f, K, shortlist, mask_seen))[1])
    res = TR.main(["--model", "SASREC", "--train", str(tmp_path / "train.tfrec"), "--valid", str(tmp_path / "valid.tfrec"), "--test",
                   str(tmp_path / "test.tfrec"), "--num_items", "300", "--num_units", "32", "--num_heads", "2", "--num_blocks", "1",
                   "--seqslen", "20", "--batch_size", "64", "--num_epochs", "1", "--mask_seen", "--dtype", "f32", "--ckpt_dir",
                   str(tmp_path / "ckpt"), "--eval_fp8_shortlist", "150"])
    assert calls and set(calls) == {150} and "H100" in res
