"""CPU-side checks of the time-independent baselines: the float64 restatement's GRU against torch.nn.GRU, the model
factory's two keys and their variable tables, the orthogonal initialiser, the host-side refusals of the GRU entry points and the
flag checks of the models.  No GPU is touched."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _seq_baselines_ref as SR


def _flags(model, **kw):
    base = dict(model=model, num_items=50, num_units=32, num_heads=2, num_blocks=2, seqslen=10, learning_rate=1e-3, l2_reg=1e-3,
                hidden_dropout_rate=0.1, attention_probs_dropout_rate=0.1, compute_dtype="f32", num_train_steps=None,
                num_warmup_steps=None)
    base.update(kw)
    return SimpleNamespace(**base)


def test_restated_gru_equals_torch_gru_in_float64():
    """The gate order r, z, n and the r * (h R_n + b_Rn) form are torch.nn.GRU's (= cuDNN's)."""
    torch.manual_seed(0)
    for B, T, I, C in ((3, 7, 5, 4), (2, 1, 8, 8)):
        g = torch.nn.GRU(I, C, batch_first=True).double()
        x = torch.randn(B, T, I, dtype=torch.float64)
        with torch.no_grad():
            want = g(x)[0]
        p = [t.detach() for t in (g.weight_ih_l0, g.bias_ih_l0, g.weight_hh_l0, g.bias_hh_l0)]
        got = SR.gru(x, p[0].t(), p[1], p[2].t(), p[3])
        assert float((got - want).abs().max()) < 1e-12
        # ... and a different gate order is a different function
        perm = torch.cat([p[2][C:2 * C], p[2][:C], p[2][2 * C:]]).t()
        assert float((SR.gru(x, p[0].t(), p[1], perm, p[3]) - want).abs().max()) > 1e-4 or T == 1


@pytest.mark.parametrize("model,shapes", [("SASREC", lambda: SR.sasrec_shapes(50, 10, 32, 2)), ("S2PNM", lambda: SR.s2pnm_shapes(50, 10, 32))])
def test_ranking_builds_both_keys_with_the_reference_names(model, shapes):
    import easydgl_amd
    m = easydgl_amd.ranking(_flags(model))
    assert type(m).__name__ == {"SASREC": "SASRec", "S2PNM": "S2PNM"}[model]
    want = shapes()
    got = m.tf_values()
    assert set(got) == set(want), set(got) ^ set(want)
    for k, sh in want.items():
        assert tuple(got[k].shape) == tuple(sh), k
    assert m.l2_param_names() == ["item_embs.lookup_table", "pcoding.pembs.lookup_table"]
    # initialisers: biases / beta zero, gamma one
    for k, v in got.items():
        leaf = k.rsplit("/", 1)[-1]
        if leaf in ("bias", "beta", "output_bias") or "/b_" in k:
            assert float(np.abs(v).max()) == 0.0, k
        if leaf == "gamma":
            assert float(v.min()) == 1.0 == float(v.max()), k
    if model == "S2PNM":
        assert m.adam_hparams == (0.9, 0.98, 1e-9) and m.clip_norm == 5.0
    else:
        assert m.adam_hparams == (0.9, 0.999, 1e-8) and m.clip_norm is None
    # a round trip through the reference's names keeps every value
    vals = {k: v + 0.01 for k, v in got.items()}
    m.sync_shadow = lambda: None       # (no arena before finalize)
    m.load_tf_variables(vals)
    back = m.tf_values()
    for k in vals:
        np.testing.assert_array_equal(back[k], vals[k].astype(np.float32))


def test_the_other_baselines_stay_refused():
    import easydgl_amd
    for name in ("GRU4REC", "BERT4REC", "GREC"):
        with pytest.raises(NotImplementedError):
            easydgl_amd.ranking(SimpleNamespace(model=name))


def test_orthogonal_initialiser_on_each_of_the_six_blocks():
    from easydgl_amd.module.coding import orthogonal_
    from easydgl_amd.module.sequential import GRU
    C = 64
    g = GRU(C, C, gen=torch.Generator().manual_seed(1))
    eye = torch.eye(C, dtype=torch.float64)
    blocks = [k[:, j * C:(j + 1) * C].detach().double() for k in (g.w_kernel, g.r_kernel) for j in range(3)]
    for q in blocks:
        assert float((q.t() @ q - eye).abs().max()) < 1e-5
    assert all(float((blocks[0] - b).abs().max()) > 0.01 for b in blocks[1:])      # six draws, not one
    assert float(g.w_bias.abs().max()) == 0.0 == float(g.r_bias.abs().max())
    # rectangular: orthonormal columns (tall) / rows (wide); the same generator state gives the same draw
    tall = orthogonal_(torch.empty(96, 32), torch.Generator().manual_seed(2)).double()
    wide = orthogonal_(torch.empty(32, 96), torch.Generator().manual_seed(2)).double()
    assert float((tall.t() @ tall - torch.eye(32, dtype=torch.float64)).abs().max()) < 1e-5
    assert float((wide @ wide.t() - torch.eye(32, dtype=torch.float64)).abs().max()) < 1e-5
    again = orthogonal_(torch.empty(96, 32), torch.Generator().manual_seed(2)).double()
    assert torch.equal(tall, again)
    with pytest.raises(ValueError):
        GRU(24)
    with pytest.raises(ValueError):
        GRU(528)


def test_gru_entry_points_refuse_bad_arguments_before_a_launch():
    from easydgl_amd import _lib
    L, one = _lib.lib, 1     # `one`: any non-null address — the checks fail before a pointer is dereferenced
    SHAPE, DTYPE, NULL = -1, -2, -4
    fwd = lambda xp=one, R=one, b=one, B=2, T=3, C=32, h=one, pack=one, dt=0: L.edgl_gru_seq_fwd(xp, R, b, B, T, C, h, None, None, pack, dt, None)
    bwd = lambda dh=one, R=one, sv=one, B=2, T=3, C=32, dxp=one, dgh=one, pack=one, dt=0: L.edgl_gru_seq_bwd(dh, R, sv, B, T, C, dxp, dgh, pack, dt, None)
    for f in (fwd, bwd):
        assert f(C=24) == SHAPE and b"bad shape" in L.edgl_last_error()
        assert f(C=528) == SHAPE
        assert f(C=0) == SHAPE
        assert f(T=0) == SHAPE
        assert f(B=0) == SHAPE
        assert f(dt=7) == DTYPE
        assert f(R=None) == NULL and b"null" in L.edgl_last_error()
        assert f(pack=None) == NULL
    assert fwd(xp=None) == NULL and fwd(b=None) == NULL and fwd(h=None) == NULL
    assert bwd(dh=None) == NULL and bwd(sv=None) == NULL and bwd(dxp=None) == NULL and bwd(dgh=None) == NULL
    # the size and path queries are host functions
    assert L.edgl_gru_seq_pack_bytes(24, 0) == -1 and L.edgl_gru_seq_pack_bytes(32, 5) == -1 and L.edgl_gru_seq_pack_bytes(528, 1) == -1
    assert L.edgl_gru_seq_pack_bytes(512, 1) == 3 * 512 * 512 * 2 and L.edgl_gru_seq_pack_bytes(128, 0) == 3 * 128 * 128 * 4
    # the LDS-resident / L2-streamed boundary DESIGN 4.17 documents
    assert [L.edgl_gru_seq_resident(c, _lib.BF16) for c in (32, 128, 144, 256, 512)] == [1, 1, 0, 0, 0]
    assert [L.edgl_gru_seq_resident(c, _lib.F32) for c in (32, 80, 96, 128, 512)] == [1, 1, 0, 0, 0]
    # S2PNM's element-wise pieces
    assert L.edgl_cat_pos_mask_fwd(None, one, one, 2, 3, 32, one, 0, None) == NULL
    assert L.edgl_cat_pos_mask_fwd(one, one, one, 2, 0, 32, one, 0, None) == SHAPE
    assert L.edgl_dict_feat_fwd(one, one, 4, 32, one, 9, None) == DTYPE
    assert L.edgl_sigmoid_bwd(one, None, one, 4, 0, None) == NULL
    assert L.edgl_clip_scale(one, 16, one, 0.0, None) == SHAPE and L.edgl_clip_scale(None, 16, one, 5.0, None) == NULL


@pytest.mark.parametrize("model", ["SASREC", "S2PNM"])
def test_models_refuse_unsupported_flags(model):
    import easydgl_amd
    for units, heads in ((50, 1), (48, 3), (1024, 8), (16, 1)):            # not a power of two in [32, 512]
        with pytest.raises(ValueError, match="num_units"):
            easydgl_amd.ranking(_flags(model, num_units=units, num_heads=heads))
    for units, heads in ((32, 4), (64, 8), (64, 3), (256, 1)):             # head dims 8, 8, none, 256
        if units // heads == 256 and model == "S2PNM":      # (a whole multiple of 128 runs sliced: S2PNM's published single head)
            easydgl_amd.ranking(_flags(model, num_units=units, num_heads=heads))
            continue
        with pytest.raises(ValueError, match="num_heads"):
            easydgl_amd.ranking(_flags(model, num_units=units, num_heads=heads))
    with pytest.raises(ValueError, match="lazy_adam"):
        easydgl_amd.ranking(_flags(model, lazy_adam=True, train_negatives=8))


@pytest.mark.parametrize("model", ["SASREC", "S2PNM"])
def test_static_engine_refuses_the_models(model):
    import easydgl_amd
    from easydgl_amd import _lib
    from easydgl_amd.engine import TrainEngine
    with pytest.raises(_lib.EdglError, match="static engine"):
        TrainEngine(easydgl_amd.ranking(_flags(model)), 4)


def test_ops_refuse_cpu_tensors():
    from easydgl_amd import _lib, ops
    from easydgl_amd.module.sequential import GRU, MultiHeadAttention
    with pytest.raises(_lib.EdglError):
        GRU(32)(torch.zeros(2, 3, 32))
    att = MultiHeadAttention(32, 2, 0.0)
    with pytest.raises(_lib.EdglError):
        att(torch.zeros(2, 3, 32), torch.zeros(2, 3, 32), False, True, ids=torch.ones(2, 3, dtype=torch.int64))
    with pytest.raises(_lib.EdglError):
        ops.clip_by_global_norm(torch.zeros(16), 5.0)
