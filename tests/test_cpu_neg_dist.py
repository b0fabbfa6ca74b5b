"""Popularity-weighted negatives with the log-Q correction, the parts that need no GPU: the alias table of
ops.build_neg_dist, the numpy replica of the weighted sampler (tests/_neg_dist_ref.py — what the GPU tests hold the kernel to), the
fp64 reference of the corrected loss, and the flag plumbing of the driver and the models."""
import inspect
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import easydgl_oracle as O
from tests import _cand_ce_ref as CE
from tests import _cand_ref as CR
from tests import _neg_dist_ref as ND

I_ = 300
BASE = ["--train", "a", "--valid", "b", "--test", "c", "--model", "EasyDGL", "--num_items", "100"]


def ops():
    from easydgl_amd import ops as _ops
    return _ops


def _zipf(I=I_):
    w = np.zeros(I)
    w[1:] = 1.0 / np.arange(1, I)
    return w


def _weights(kind):
    if kind == "uniform":
        w = np.ones(I_)
    elif kind == "dominant":
        w = np.ones(I_)
        w[7] = 100.0                                         # 100 / 398 of the weight: a quarter
    else:
        w = _zipf()
    w[0] = np.nan                                            # outside [1, I): ignored
    return w


# ---- the table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "dominant", "zipf"])
def test_table_implies_the_weights(kind):
    w = _weights(kind)
    d = ops().build_neg_dist(w, 1, I_, 0)
    n = I_ - 1
    assert d.thr.dtype == np.uint32 and d.alias.dtype == np.int32 and d.thr.shape == d.alias.shape == (n,)
    assert d.logq.dtype == np.float32 and d.logq.shape == (I_,) and (d.lo, d.hi, d.T_reject) == (1, I_, 0)
    assert ((d.alias >= 0) & (d.alias < n)).all()
    target = w[1:] / w[1:].sum()
    got = ND.implied(d.thr, d.alias)
    err = float(np.abs(got - target).max())
    print(kind, "max |implied - target|", err, "bound", n * 2.0 ** -32)
    assert err <= n * 2.0 ** -32
    assert np.array_equal(got, d.probabilities())
    if kind == "uniform":
        assert np.array_equal(d.alias, np.arange(n))         # every bucket full: either branch returns the bucket
    else:
        assert (d.alias != np.arange(n)).sum() >= n // 2
        full = d.alias == np.arange(n)
        assert (d.thr[~full].astype(np.uint64) < 2 ** 32).all()
    assert d.logq[0] == 0.0
    assert np.array_equal(d.logq[1:], np.log(target).astype(np.float32))          # fp64, rounded once
    again = ops().build_neg_dist(w.astype(np.float64), 1, I_, 0)
    assert np.array_equal(again.thr, d.thr) and np.array_equal(again.alias, d.alias)        # a fixed build order


def test_a_sub_range_ignores_everything_outside():
    w = _zipf()
    a = ops().build_neg_dist(w, 10, 200, 3)
    w2 = w.copy()
    w2[:10], w2[200:] = -1.0, np.inf
    b = ops().build_neg_dist(w2, 10, 200, 3)
    assert np.array_equal(a.thr, b.thr) and np.array_equal(a.alias, b.alias) and np.array_equal(a.logq, b.logq)
    assert not a.logq[:10].any() and not a.logq[200:].any() and (a.logq[10:200] < 0).all()
    assert abs(float(np.exp(a.logq[10:200].astype(np.float64)).sum()) - 1.0) < 1e-5


def test_refusals_of_the_table_build():
    for bad in (0.0, -1.0, np.nan, np.inf):
        w = np.ones(I_)
        w[17] = bad
        with pytest.raises(ValueError, match=r"id 17: every weight of \[1, 300\) must be finite and > 0"):
            ops().build_neg_dist(w, 1, I_, 0)
    # the half-mass rule, the weighted form of 2 (T + 1) <= hi - lo
    w = np.ones(I_)
    w[5] = 299.0                                             # 299 of 597: just past half
    with pytest.raises(ValueError, match=r"T_reject \+ 1 = 1 heaviest ids .* more than 1/2: .* probability <= 1/2"):
        ops().build_neg_dist(w, 1, I_, 0)
    w[5] = 298.0                                             # exactly half: the bound holds
    ops().build_neg_dist(w, 1, I_, 0)
    z = _zipf()
    ops().build_neg_dist(z, 1, I_, 8)                        # H_9 / H_299 = 0.45
    with pytest.raises(ValueError, match=r"T_reject \+ 1 = 13 heaviest ids"):
        ops().build_neg_dist(z, 1, I_, 12)                   # H_13 / H_299 = 0.506
    u = np.ones(I_)
    ops().build_neg_dist(u, 1, 19, 8)                        # uniform, hi - lo = 2 (T + 1): the tightest legal range
    with pytest.raises(ValueError, match="more than 1/2"):
        ops().build_neg_dist(u, 1, 18, 8)
    with pytest.raises(ValueError, match="1 <= lo < hi <= I"):
        ops().build_neg_dist(u, 0, 10, 0)
    with pytest.raises(ValueError, match="float64 / float32"):
        ops().build_neg_dist(np.ones(I_, dtype=np.int64), 1, I_, 0)


def test_weight_presets():
    cnt = np.array([9, 0, 3, 15, 1])
    w = ops().neg_weights("popularity", 6, 1, 5, cnt, 0.75)
    assert w.shape == (6,) and w[0] == 0.0 and w[5] == 0.0
    assert np.allclose(w[1:5], (cnt[1:5] + 1.0) ** 0.75) and (w[1:5] > 0).all()       # add-one: a count of 0 keeps a weight
    lu = ops().neg_weights("log_uniform", 10, 2, 9)
    k = np.arange(7)
    assert np.allclose(lu[2:9], np.log((k + 2.0) / (k + 1.0))) and not lu[:2].any() and lu[9] == 0.0
    assert abs(lu[2:9].sum() - np.log(8.0)) < 1e-12          # telescopes: TensorFlow's log(range + 1) normaliser
    with pytest.raises(ValueError, match="counts"):
        ops().neg_weights("popularity", 6, 1, 5)
    with pytest.raises(ValueError, match="sampler"):
        ops().neg_weights("unigram", 6, 1, 5)


# ---- the replica sampler -----------------------------------------------------------------------------------------------------------
def test_replica_sampler_follows_the_weights():
    """Zipf(1) over the 299 ids of I = 300, 200 rows of 1000 slots, seed 7 (the first seed tried), K = 0x68E31DA4: neighbouring ids
    merged to bins that expect >= 1 / 50 of the draws; chi^2 below the 99.9 % quantile (32 bins: 21.8 against 61.1)."""
    w = _zipf()
    d = ops().build_neg_dist(w, 1, I_, 0)
    ids, worst = ND.sample_negatives(None, np.zeros(200, dtype=np.int64), 1000, 1, I_, 7, d.thr, d.alias)
    assert worst == 1 and (ids >= 1).all() and (ids < I_).all()                  # nothing banned: the first attempt stands
    target = w[1:] / w[1:].sum()
    x2, bins = ND.chi2_against(ids, 1, target)
    q = ND.chi2_quantile(0.999, bins - 1)
    print("chi2", x2, "bins", bins, "99.9 % quantile", q)
    assert abs(ND.chi2_quantile(0.999, 31) - 61.098) < 0.01                       # (the tabulated value)
    assert 20 <= bins <= 50 and x2 < q
    # ... and not the uniform distribution: the same draws against uniform weights fail by a wide margin
    assert ND.chi2_against(ids, 1, np.full(I_ - 1, 1.0 / (I_ - 1)))[0] > 100 * q


def test_replica_leaves_no_slot_empty_at_the_half_mass_bound():
    """The 8 heaviest ids seen, the 9th the label: 0.45 of the weight is rejected; 130 rows of 257 slots."""
    w = _zipf()
    d = ops().build_neg_dist(w, 1, I_, 8)
    seen = np.tile(np.arange(1, 9), (130, 1))
    labels = np.full(130, 9)
    ids, worst = ND.sample_negatives(seen, labels, 257, 1, I_, 7, d.thr, d.alias)
    print("worst attempt", worst)
    assert (ids >= 10).all() and worst <= 32
    # the draws that survive follow the weights renormalised over the ids that are left
    t = w[10:] / w[10:].sum()
    x2, bins = ND.chi2_against(ids, 10, t)
    assert x2 < ND.chi2_quantile(0.999, bins - 1)


def test_replica_keys():
    """Rows, steps and row0 move the lists as in the uniform sampler; the attempt word is the uniform sampler's."""
    d = ops().build_neg_dist(_zipf(), 1, I_, 0)
    lab = np.array([3, 4, 5])
    a, _ = ND.sample_negatives(None, lab, 16, 1, I_, 7, d.thr, d.alias, step=2)
    b, _ = ND.sample_negatives(None, lab[1:], 16, 1, I_, 7, d.thr, d.alias, step=2, row0=1)
    assert np.array_equal(a[1:], b)
    c, _ = ND.sample_negatives(None, lab, 16, 1, I_, 7, d.thr, d.alias, step=3)
    assert not np.array_equal(a, c)
    k = CR.sampler_key(7, 2)
    h = ND.attempt_word(k, 1, np.arange(16), 0)
    assert np.array_equal(CR.draw(k, 1, np.arange(16), 0, 1, I_), 1 + ((h * np.uint64(I_ - 1)) >> np.uint64(32)).astype(np.int64))


# ---- the corrected loss --------------------------------------------------------------------------------------------------------------
def test_reference_is_a_bias_shift():
    rng = np.random.default_rng(0)
    R, C, N, I = 6, 16, 9, 40
    rows, table, bias = rng.standard_normal((R, C)), rng.standard_normal((I, C)), rng.standard_normal(I - 1) * 0.3
    lab = rng.integers(1, I, size=R)
    lab[2] = 0
    cand = rng.integers(1, I, size=(R, N))
    cand[0, 0], cand[1, 1], cand[3, 2], cand[4, 3] = -1, lab[1], 0, cand[4, 4]
    w = np.zeros(I)
    w[1:] = rng.random(I - 1) + 0.1
    logq = np.zeros(I)
    logq[1:] = np.log(w[1:] / w[1:].sum())
    ref = ND.reference(rows, table, bias, logq, cand, lab)
    # from the definition: v' = v - logq[c] on the label and every live slot
    tu, bu = CE.used(table, bias)
    terms = []
    for r in range(R):
        if lab[r] == 0:
            continue
        ids, _ = CE.slots(cand[r], lab[r], I)
        v = tu[ids] @ rows[r] + bu[ids] - logq[ids]
        p = np.exp(v - v.max())
        terms.append(-np.log(p[0] / p.sum() + 1e-5))
    want = sum(terms) / (len(terms) + 1e-5)
    assert abs(ref["loss"] - want) <= 1e-12 * abs(want)
    zero = ND.reference(rows, table, bias, np.zeros(I), cand, lab)
    plain = CE.reference(rows, table, bias, cand, lab)
    for k in ("loss", "lse", "d_rows", "d_table", "d_bias"):
        assert np.array_equal(zero[k], plain[k])
    assert abs(ref["loss"] - plain["loss"]) > 1e-3           # the correction is at work
    # a constant logq cancels: the uniform sampler needs no correction
    const = np.concatenate([[0.0], np.full(I - 1, -3.5)])
    nz = cand.copy()
    nz[nz == 0] = 1
    a, b = ND.reference(rows, table, bias, const, nz, lab), CE.reference(rows, table, bias, nz, lab)
    assert abs(a["loss"] - b["loss"]) <= 1e-12 and np.allclose(a["d_rows"], b["d_rows"], atol=1e-14)


# ---- flags and signatures ------------------------------------------------------------------------------------------------------------
def test_driver_flags(capsys):
    from easydgl_amd import train
    a = train.args(BASE)
    assert a.neg_sampler == "uniform" and a.neg_alpha == 0.75 and a.eval_neg_sampler == "uniform"
    a = train.args(BASE + ["--train_negatives", "8", "--neg_sampler", "popularity", "--neg_alpha", "0.5"])
    assert a.neg_sampler == "popularity" and a.neg_alpha == 0.5
    a = train.args(BASE + ["--shared_negatives", "64", "--neg_sampler", "log_uniform", "--lazy_adam", "--deterministic"])
    assert a.neg_sampler == "log_uniform" and a.lazy_adam and a.deterministic
    a = train.args(BASE + ["--eval_negatives", "100", "--eval_neg_sampler", "popularity"])
    assert a.eval_neg_sampler == "popularity" and a.neg_sampler == "uniform"
    with pytest.raises(SystemExit):
        train.args(BASE + ["--neg_sampler", "popularity"])
    err = capsys.readouterr().err
    assert "--train_negatives" in err and "--shared_negatives" in err
    with pytest.raises(SystemExit):
        train.args(BASE + ["--eval_neg_sampler", "popularity"])
    assert "--eval_negatives" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.args(BASE + ["--train_negatives", "8", "--neg_sampler", "unigram"])
    with pytest.raises(SystemExit):                          # the static engine / graph refusals stand
        train.args(BASE + ["--train_negatives", "8", "--neg_sampler", "popularity", "--graph"])
    assert inspect.signature(train.evaluate).parameters["neg_dist"].default is None


def _flags(model, **kw):
    F = SimpleNamespace(model=model, num_items=50, num_units=32, num_heads=2, num_blocks=1, seqslen=8, masklen=2, timelen=32,
                        time_scale=86400.0, learning_rate=1e-3, l2_reg=0.0, ct_reg=0.0, hidden_dropout_rate=0.0,
                        attention_probs_dropout_rate=0.0, mark_table=O.synthetic_mark_table(50, 4), compute_dtype="f32",
                        num_train_steps=None, num_warmup_steps=None)
    for k, v in kw.items():
        setattr(F, k, v)
    return F


def test_models_take_the_flags():
    import easydgl_amd
    from easydgl_amd import engine
    from easydgl_amd.model import base, ctsma, easydgl, tgat, tisasrec
    from easydgl_amd.model.base import Sequential
    assert base.NEG_SAMPLERS == ("uniform", "popularity", "log_uniform")
    for mod in (ctsma, easydgl, tgat, tisasrec):             # read in one place, for all four
        assert "neg_sampler" not in inspect.getsource(mod)
    for name in ("EasyDGL", "CTSMA", "TGAT", "TiSASREC"):
        m = easydgl_amd.ranking(_flags(name))
        assert m.neg_sampler == "uniform" and m.neg_alpha == 0.75 and m._negative_dist() is None
        m = easydgl_amd.ranking(_flags(name, train_negatives=8, neg_sampler="popularity", neg_alpha=0.5))
        assert m.neg_sampler == "popularity" and m.neg_alpha == 0.5 and m.train_negatives == 8
        with pytest.raises(ValueError, match=r"call model\.set_negative_weights\(weights\)"):
            m._negative_dist()                               # what the first draw asks for
        hi = m._negatives_hi()
        m.set_negative_weights(ops().neg_weights("popularity", hi, 1, hi, np.arange(hi), m.neg_alpha))
        d = m._negative_dist()
        rows = m.item_embs.lookup_table.shape[0]
        assert (d.lo, d.hi, d.T_reject) == (1, hi, 0) and d.logq.shape == (rows,) and not d.logq[hi:].any()
        want = (np.arange(1, hi) + 1.0) ** 0.5
        assert np.allclose(np.exp(d.logq[1:hi].astype(np.float64)), want / want.sum(), rtol=1e-6)
        with pytest.raises(ValueError, match="one per item id"):
            m.set_negative_weights(np.ones(hi - 1))
        with pytest.raises(ValueError, match="finite and > 0"):
            m.set_negative_weights(np.zeros(hi))
        ev = m.negative_dist(np.ones(hi), T_reject=8)        # the evaluation's table: the history and the label are rejected
        assert ev.T_reject == 8 and m._negative_dist() is d
        # log_uniform needs nothing but the range
        m = easydgl_amd.ranking(_flags(name, shared_negatives=16, neg_sampler="log_uniform"))
        d = m._negative_dist()
        k = np.arange(hi - 1)
        assert np.allclose(np.exp(d.logq[1:hi].astype(np.float64)), np.log((k + 2.0) / (k + 1.0)) / np.log(hi), rtol=1e-6)
        for kw in (dict(neg_sampler="popularity"), dict(neg_sampler="log_uniform")):
            with pytest.raises(ValueError, match="needs train_negatives > 0 or shared_negatives > 0"):
                easydgl_amd.ranking(_flags(name, **kw))
        with pytest.raises(ValueError, match="neg_sampler='unigram'"):
            easydgl_amd.ranking(_flags(name, train_negatives=8, neg_sampler="unigram"))
        with pytest.raises(ValueError, match="uniform"):
            easydgl_amd.ranking(_flags(name, train_negatives=8)).set_negative_weights(np.ones(hi))
        with pytest.raises(ValueError, match="train_step"):  # sampled modes stay off the captured graph
            m.graphed_train_step({}, None)
    assert easydgl_amd.ranking(_flags("EasyDGL", shared_negatives=16, neg_sampler="log_uniform", lazy_adam=True,
                                      deterministic=True)).lazy_adam
    assert list(inspect.signature(Sequential._score_ce).parameters)[-2:] == ["candidates", "shared"]
    assert "model.train_step" in inspect.getsource(engine.TrainEngine.__init__)
    par = inspect.signature(Sequential.eval_step).parameters
    assert par["neg_dist"].kind is inspect.Parameter.KEYWORD_ONLY and par["neg_dist"].default is None
    assert inspect.signature(Sequential.eval_candidates).parameters["dist"].default is None


def test_op_signatures():
    o = ops()
    assert inspect.signature(o.sample_negatives).parameters["dist"].default is None
    assert list(inspect.signature(o.sample_negatives).parameters)[:8] == ["seen", "labels", "n", "lo", "hi", "seed", "step", "row0"]
    for f in (o.cand_ce_fwd, o.shared_ce_fwd):
        assert list(inspect.signature(f).parameters)[-1] == "logq" and inspect.signature(f).parameters["logq"].default is None
    for fn in (o.SampledCEFn, o.SharedCEFn):
        par = inspect.signature(fn.forward).parameters
        assert list(par)[-2:] == ["d_table_out", "logq"] and par["logq"].default is None
    from easydgl_amd import _lib
    for name in ("edgl_sample_negatives_alias", "edgl_cand_ce_fwd_q", "edgl_shared_ce_fwd_q"):
        assert hasattr(_lib.lib, name)
    hdr = open(_lib.__file__.replace("easydgl_amd/_lib.py", "include/easydgl_hip.h")).read()
    for name in ("edgl_sample_negatives_alias(", "edgl_cand_ce_fwd_q(", "edgl_shared_ce_fwd_q(", "0x68E31DA4"):
        assert name in hdr


def test_entry_points_check_before_any_launch():
    from easydgl_amd import _lib
    L, ONE = _lib.lib, 16
    assert L.edgl_sample_negatives_alias(None, 0, None, 1, 4, 1, 100, 100, None, 0, 0, 0, ONE, None) == -4
    assert b"null" in L.edgl_last_error()
    assert L.edgl_sample_negatives_alias(None, 3, None, 1, 4, 1, 100, 100, ONE, 0, 0, 0, ONE, None) == -4
    assert b"without seen ids" in L.edgl_last_error()
    assert L.edgl_sample_negatives_alias(None, 0, None, 1, 4, 0, 100, 100, ONE, 0, 0, 0, ONE, None) == -1
    assert b"1 <= lo < hi <= I" in L.edgl_last_error()
    assert L.edgl_sample_negatives_alias(None, 0, None, 1, 0, 1, 100, 100, ONE, 0, 0, 0, ONE, None) == -1
    assert L.edgl_sample_negatives_alias(ONE, 1025, None, 1, 4, 1, 100, 100, ONE, 0, 0, 0, ONE, None) == -1
    assert b"0 <= T <= 1024" in L.edgl_last_error()
    assert L.edgl_sample_negatives_alias(None, 0, None, 1, 4, 1, 100, 100, 20, 0, 0, 0, ONE, None) == -1
    assert b"8-byte aligned" in L.edgl_last_error()
    assert L.edgl_cand_ce_fwd_q(ONE, ONE, ONE, ONE, ONE, ONE, 4, 24, 100, 10, ONE, ONE, ONE, 0, None) == -1
    assert b"multiple of 16" in L.edgl_last_error()
    assert L.edgl_cand_ce_fwd_q(ONE, ONE, ONE, None, ONE, ONE, 4, 64, 100, 10, None, ONE, ONE, 0, None) == -4
    assert L.edgl_shared_ce_fwd_q(ONE, ONE, ONE, ONE, ONE, ONE, None, 4, 64, 100, 0, ONE, ONE, ONE, 0, None) == -1
    assert b"1 <= S <= 8192" in L.edgl_last_error()
    assert L.edgl_shared_ce_fwd_q(ONE, ONE, ONE, None, ONE, ONE, None, 4, 64, 100, 10, None, ONE, ONE, 0, None) == -4


def test_checkpoint_keeps_the_sampler(tmp_path):
    """The checkpoint names the sampler and its exponent; a resume under other values is refused before anything is copied."""
    import torch
    from easydgl_amd import train as TR

    def fake(sampler, alpha):
        z = torch.zeros(4)
        return SimpleNamespace(_arena=z.clone(), _adam_m=z.clone(), _adam_v=z.clone(), _adam_state=z.clone(), _rng_state=z.clone(),
                               _offsets={"w": (0, 4)}, neg_step=3, neg_sampler=sampler, neg_alpha=alpha, lazy_adam=False,
                               settle_state=lambda: None, sync_shadow=lambda: None)
    path = str(tmp_path / "m.pt")
    TR.save_checkpoint(fake("popularity", 0.75), path)
    ck = torch.load(path, map_location="cpu")
    assert ck["neg_sampler"] == "popularity" and ck["neg_alpha"] == 0.75 and ck["neg_step"] == 3
    m = fake("popularity", 0.75)
    m.neg_step = 0
    TR.load_checkpoint(m, path)
    assert m.neg_step == 3
    for other in (fake("uniform", 0.75), fake("log_uniform", 0.75), fake("popularity", 0.5)):
        with pytest.raises(ValueError, match="a resumed run keeps its negative sampler"):
            TR.load_checkpoint(other, path)
    # a checkpoint from before the fields existed is a uniform run
    del ck["neg_sampler"], ck["neg_alpha"]
    torch.save(ck, str(tmp_path / "old.pt"))
    TR.load_checkpoint(fake("uniform", 0.75), str(tmp_path / "old.pt"))
    with pytest.raises(ValueError, match="neg_sampler='uniform'"):
        TR.load_checkpoint(fake("popularity", 0.75), str(tmp_path / "old.pt"))
