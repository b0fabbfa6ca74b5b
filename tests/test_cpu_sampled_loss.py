"""Binary cross-entropy and BPR over sampled negatives, the parts that need no GPU: the fp64 restatement the GPU tests
hold the kernels to (tests/_sampled_loss_ref.py) against the closed forms of the definition, the flag on the models and the driver,
the checkpoint field, and the entry points' refusals before any launch."""
import inspect
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import easydgl_oracle as O
from tests import _cand_ce_ref as CE
from tests import _sampled_loss_ref as SL

ONE = 16      # any non-null, 16-byte aligned address: the checks below fail before a pointer is dereferenced


def _problem(R, C, I, N, seed):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((R, C)) * 0.5
    table = rng.standard_normal((I, C)) * 0.5
    bias = rng.standard_normal(I - 1) * 0.3
    cand = rng.integers(1, I, size=(R, N))
    labels = rng.integers(1, I, size=R)
    return rows, table, bias, cand, labels


def _edge_problem(seed=1):
    R, C, I, N = 6, 16, 12, 5
    rows, table, bias, cand, labels = _problem(R, C, I, N, seed)
    cand[0, 1] = -1                   # empty slot
    cand[0, 2] = labels[0]            # accidental hit
    cand[1, 0] = 0                    # item 0: the zero row with bias -1000
    cand[1, 3] = I + 2                # past the table
    cand[2, 1] = cand[2, 4]           # a repeated id
    cand[3] = [-1, labels[3], I, -1, I + 7]      # every slot dead
    labels[4] = 0                     # weight 0
    labels[5] = I                     # a label outside the table: weight 0
    return rows, table, bias, cand, labels


def _closed_form(ref, rows, table, bias, labels, form, g):
    """d_rows / d_table / d_bias from the dv of the definition, over the restatement's own values."""
    R, C = rows.shape
    I = table.shape[0]
    tu, _ = CE.used(table, bias)
    d_rows, d_table, d_bu = np.zeros((R, C)), np.zeros((I, C)), np.zeros(I)
    W = ref["weight"] + 1e-5
    dvs = []
    for r in range(R):
        v, ids = ref["values"][r], ref["ids"][r]
        if v is None:
            dvs.append(None)
            continue
        dv = np.zeros(len(v))
        if form == "bce":
            dv[0] = SL.sigmoid(v[0]) - 1.0
            dv[1:] = SL.sigmoid(v[1:])
        else:
            n = len(v) - 1
            if n:
                dv[1:] = SL.sigmoid(v[1:] - v[0]) / n
                dv[0] = -dv[1:].sum()
        dv *= g / W
        dvs.append(dv)
        d_rows[r] = dv @ tu[ids]
        np.add.at(d_table, ids, dv[:, None] * rows[r][None, :])
        np.add.at(d_bu, ids, dv)
    d_table[0] = 0.0
    return d_rows, d_table, d_bu[1:], dvs


@pytest.mark.parametrize("form", ["bce", "bpr"])
@pytest.mark.parametrize("shared", [False, True])
def test_autograd_gradients_equal_the_closed_forms(form, shared):
    rows, table, bias, cand, labels = _edge_problem()
    lists = np.array([3, -1, 0, int(labels[0]), 40, 7, 7]) if shared else cand
    rng = np.random.default_rng(9)
    logq = np.concatenate([[0.0], np.log(rng.uniform(0.01, 0.2, size=table.shape[0] - 1))])
    for lq in (None, logq):
        ref = SL.reference(rows, table, bias, labels, lists, lq, form, g=0.7)
        d_rows, d_table, d_bias, dvs = _closed_form(ref, rows, table, bias, labels, form, 0.7)
        for got, want, what in ((ref["d_rows"], d_rows, "d_rows"), (ref["d_table"], d_table, "d_table"), (ref["d_bias"], d_bias, "d_bias")):
            assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), (form, shared, what)
        assert np.abs(ref["d_rows"]).max() > 1e-3 and not ref["d_table"][0].any()
        assert ref["weight"] == 4 and not ref["d_rows"][4:].any() and not ref["row_loss"][4:].any()
        if form == "bpr":                                    # the pairwise loss moves the label against its negatives: sum dv = 0
            for dv in dvs:
                if dv is not None:
                    assert abs(dv.sum()) <= 1e-15
        if lq is not None:                                   # the term is subtracted from the label's and every slot's value
            plain = SL.reference(rows, table, bias, labels, lists, None, form)
            assert np.allclose(ref["values"][0], plain["values"][0] - logq[ref["ids"][0]], rtol=0, atol=1e-12)


def test_bce_with_one_negative_is_sasrecs_loss():
    rows, table, bias, cand, labels = _problem(5, 16, 30, 1, 3)
    cand[:, 0] = (labels + 3) % 29 + 1                       # one live negative per row, never the label
    assert not (cand[:, 0] == labels).any()
    ref = SL.reference(rows, table, bias, labels, cand, None, "bce")
    want = np.array([-np.log(SL.sigmoid(v[0])) - np.log(1.0 - SL.sigmoid(v[1])) for v in ref["values"]])
    assert np.abs(ref["row_loss"] - want).max() <= 1e-13
    assert ref["loss"] == pytest.approx(want.sum() / (5 + 1e-5), rel=1e-13)


@pytest.mark.parametrize("form", ["bce", "bpr"])
def test_an_all_dead_row_gives_no_nan(form):
    rows, table, bias, cand, labels = _edge_problem()
    ref = SL.reference(rows, table, bias, labels, cand, None, form)
    assert len(ref["values"][3]) == 1                        # the label alone
    for k in ("row_loss", "d_rows", "d_table", "d_bias"):
        assert np.isfinite(ref[k]).all(), k
    if form == "bpr":
        assert ref["row_loss"][3] == 0.0 and not ref["d_rows"][3].any()
    else:                                                    # bce keeps the label's term
        assert ref["row_loss"][3] == pytest.approx(np.log1p(np.exp(-ref["values"][3][0])), rel=1e-13)
    only = SL.reference(rows[3:4], table, bias, labels[3:4], cand[3:4], None, form)
    assert np.isfinite(only["loss"]) and np.isfinite(only["d_table"]).all()


def test_softmax_through_the_restatement_is_the_softmax_reference():
    rows, table, bias, cand, labels = _edge_problem()
    labels[5] = 0                                            # (_cand_ce_ref weighs by label != 0: keep the labels inside the table)
    a = SL.reference(rows, table, bias, labels, cand, None, "softmax", g=1.3)
    b = CE.reference(rows, table, bias, cand, labels, g=1.3)
    assert a["loss"] == pytest.approx(b["loss"], rel=1e-13)
    for k in ("d_rows", "d_table", "d_bias"):
        assert np.abs(a[k] - b[k]).max() <= 1e-13 * np.abs(b[k]).max(), k
    assert np.abs(a["row_loss"] - b["terms"]).max() <= 1e-13


def test_the_restatement_does_not_import_the_package():
    assert "easydgl_amd" not in inspect.getsource(SL)


# ---- the flag ------------------------------------------------------------------------------------------------------------------------
def _flags(model, **kw):
    F = SimpleNamespace(model=model, num_items=50, num_units=32, num_heads=2, num_blocks=1, seqslen=8, masklen=2, timelen=32,
                        time_scale=86400.0, learning_rate=1e-3, l2_reg=0.0, ct_reg=0.0, hidden_dropout_rate=0.0,
                        attention_probs_dropout_rate=0.0, mark_table=O.synthetic_mark_table(50, 4), compute_dtype="f32",
                        num_train_steps=None, num_warmup_steps=None)
    for k, v in kw.items():
        setattr(F, k, v)
    return F


@pytest.mark.parametrize("name", ["EasyDGL", "SASREC", "TiSASREC", "TGAT"])
def test_models_read_the_flag(name):
    import easydgl_amd
    assert easydgl_amd.ranking(_flags(name)).sampled_loss == "softmax"
    assert easydgl_amd.ranking(_flags(name, sampled_loss=None, train_negatives=4)).sampled_loss == "softmax"
    for form in ("bce", "bpr"):
        assert easydgl_amd.ranking(_flags(name, sampled_loss=form, train_negatives=4)).sampled_loss == form
        assert easydgl_amd.ranking(_flags(name, sampled_loss=form, shared_negatives=8)).sampled_loss == form
        with pytest.raises(ValueError, match="sampled_loss=.*needs train_negatives > 0 or shared_negatives > 0"):
            easydgl_amd.ranking(_flags(name, sampled_loss=form))
    with pytest.raises(ValueError, match="sampled_loss='hinge'"):
        easydgl_amd.ranking(_flags(name, sampled_loss="hinge", train_negatives=4))
    m = easydgl_amd.ranking(_flags(name, sampled_loss="bce", train_negatives=4))
    with pytest.raises(ValueError, match="train_step"):      # sampled modes stay off the captured graph
        m.graphed_train_step({}, None)


def test_lazy_adam_and_deterministic_take_the_flag():
    import easydgl_amd
    m = easydgl_amd.ranking(_flags("EasyDGL", sampled_loss="bpr", shared_negatives=8, lazy_adam=True, deterministic=True,
                                   neg_sampler="log_uniform"))
    assert m.lazy_adam and m.deterministic and m.sampled_loss == "bpr"


def test_op_signatures_and_symbols():
    from easydgl_amd import _lib, ops
    assert ops.LOSS_FORMS == {"softmax": 0, "bce": 1, "bpr": 2}
    for fn in (ops.SampledCEFn, ops.SharedCEFn):
        # forward keeps the nine arguments other tests pin; the objective is `.apply`'s tenth (or form=) and picks a variant
        assert list(inspect.signature(fn.forward).parameters)[-2:] == ["d_table_out", "logq"]
        assert list(inspect.signature(fn.apply).parameters) == ["args", "form"]
        for form in ("bce", "bpr"):
            v = ops._form_variant(fn, form)
            assert issubclass(v, fn) and v is ops._form_variant(fn, form) and v.backward is fn.backward and form in v.__name__
        with pytest.raises(ValueError, match="form must be one of"):
            fn.apply(*[None] * 9, "hinge")
        with pytest.raises(ValueError, match="form must be one of"):
            fn.apply(*[None] * 7, form="hinge")
        with pytest.raises(TypeError, match="at most ten"):
            fn.apply(*[None] * 10, "bce")
    hdr = open(_lib.__file__.replace("easydgl_amd/_lib.py", "include/easydgl_hip.h")).read()
    for name in ("edgl_sampled_row_loss", "edgl_sampled_loss_finish", "edgl_cand_ce_bwd_form", "edgl_shared_ce_bwd_form"):
        assert hasattr(_lib.lib, name) and name + "(" in hdr
    with pytest.raises(ValueError, match="form must be one of"):
        ops._loss_form("hinge", "test")


def test_entry_points_refuse_before_any_launch():
    from easydgl_amd import _lib
    L = _lib.lib

    def row(R=4, S=10, I=100, form=1, vals=ONE):
        return L.edgl_sampled_row_loss(vals, None, ONE, None, R, S, I, form, ONE, ONE, ONE, None)

    def cand(form=1, C=64, N=10):
        return L.edgl_cand_ce_bwd_form(ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, None, 4, C, 100, N, ONE, ONE, ONE, ONE, form, 1, None)

    def shared(form=1, C=64, S=10, ws=ONE):
        return L.edgl_shared_ce_bwd_form(ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, None, None, 4, C, 100, S, ONE, ONE, ONE, ws, None,
                                         None, form, 1, None)
    for bad in (0, 3, -1):                                   # (the softmax loss is edgl_ce_loss_fwd's: no row-loss form 0)
        assert row(form=bad) == -1 and b"bce = 1 or bpr = 2" in L.edgl_last_error()
    assert row(S=0) == -1 and b"1 <= S <= 8192" in L.edgl_last_error()
    assert row(S=8193) == -1 and row(R=0) == -1 and row(I=1) == -1
    assert row(R=1 << 20, S=1 << 12) == -1 and b"2^31" in L.edgl_last_error()
    assert row(vals=None) == -4 and b"null" in L.edgl_last_error()
    assert L.edgl_sampled_loss_finish(ONE, ONE, ONE, None, 0, 100, ONE, ONE, None) == -1 and b"R >= 1" in L.edgl_last_error()
    assert L.edgl_sampled_loss_finish(ONE, ONE, ONE, None, 4, 100, None, ONE, None) == -4
    for call in (cand, shared):
        for bad in (3, -1):
            assert call(form=bad) == -1 and b"0 <= form <= 2" in L.edgl_last_error()
        assert call(C=520) == -1 and b"512" in L.edgl_last_error()
    assert cand(N=0) == -1 and b"1 <= N <= 8192" in L.edgl_last_error()
    assert shared(S=0) == -1 and b"1 <= S <= 8192" in L.edgl_last_error()
    assert shared(ws=None) == -5 and b"edgl_shared_ce_workspace" in L.edgl_last_error()


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
BASE = ["--train", "a", "--valid", "b", "--test", "c", "--model", "TiSASREC", "--num_items", "100"]


def test_driver_takes_the_flag_and_refuses_it_without_negatives(capsys):
    from easydgl_amd import train
    assert train.args(BASE).sampled_loss == "softmax"
    assert train.args(BASE + ["--sampled_loss", "bce", "--train_negatives", "1"]).sampled_loss == "bce"
    assert train.args(BASE + ["--sampled_loss", "bpr", "--shared_negatives", "64", "--neg_sampler", "log_uniform"]).sampled_loss == "bpr"
    assert train.args(BASE + ["--sampled_loss", "softmax"]).sampled_loss == "softmax"
    with pytest.raises(SystemExit):
        train.args(BASE + ["--sampled_loss", "bce"])
    err = capsys.readouterr().err
    assert "--train_negatives" in err and "--shared_negatives" in err
    with pytest.raises(SystemExit):
        train.args(BASE + ["--sampled_loss", "hinge", "--train_negatives", "4"])
    with pytest.raises(SystemExit):                          # the graph refusal stands
        train.args(BASE + ["--sampled_loss", "bce", "--train_negatives", "4", "--graph"])


def test_checkpoint_keeps_the_objective(tmp_path):
    import torch
    from easydgl_amd import train as TR

    def fake(form):
        z = torch.zeros(4)
        return SimpleNamespace(_arena=z.clone(), _adam_m=z.clone(), _adam_v=z.clone(), _adam_state=z.clone(), _rng_state=z.clone(),
                               _offsets={"w": (0, 4)}, neg_step=3, neg_sampler="uniform", neg_alpha=0.75, sampled_loss=form,
                               lazy_adam=False, settle_state=lambda: None, sync_shadow=lambda: None)
    path = str(tmp_path / "m.pt")
    TR.save_checkpoint(fake("bce"), path)
    ck = torch.load(path, map_location="cpu")
    assert ck["sampled_loss"] == "bce"
    m = fake("bce")
    m.neg_step = 0
    TR.load_checkpoint(m, path)
    assert m.neg_step == 3
    for other in ("softmax", "bpr"):
        with pytest.raises(ValueError, match="a resumed run keeps its objective"):
            TR.load_checkpoint(fake(other), path)
    del ck["sampled_loss"]                                   # a checkpoint from before the field existed: a softmax run
    torch.save(ck, str(tmp_path / "old.pt"))
    TR.load_checkpoint(fake("softmax"), str(tmp_path / "old.pt"))
    with pytest.raises(ValueError, match="sampled_loss='softmax'"):
        TR.load_checkpoint(fake("bce"), str(tmp_path / "old.pt"))
