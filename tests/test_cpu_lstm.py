"""The LSTM form of the recurrent layer without a GPU: argument checks of the three entry points (no call reaches a
launch), the initialisers of module.sequential.LSTM, GRU4REC's variable table with rnn_cell="lstm", and the refusals."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _gru4rec_lstm_ref as LR
from tests import _seq_baselines_ref as SR
from tests.test_cpu_gru4rec import _model


def test_entry_points_refuse_bad_arguments_before_a_launch():
    from easydgl_amd import _lib
    L, one = _lib.lib, 1      # `one`: any non-null address — the checks fail before a pointer is dereferenced
    fwd = lambda xp=one, R=one, bR=one, B=2, T=3, C=32, h=one, pack=one, dt=0: L.edgl_lstm_seq_fwd(xp, R, bR, B, T, C, h, None, None, pack,
                                                                                                   dt, None)
    bwd = lambda dh=one, R=one, sv=one, B=2, T=3, C=32, dxp=one, pack=one, dt=0: L.edgl_lstm_seq_bwd(dh, R, sv, B, T, C, dxp, pack, dt, None)
    for call in (fwd, bwd):
        for bad in (dict(C=24), dict(C=528), dict(C=0), dict(T=0), dict(B=0)):
            assert call(**bad) == -1 and b"multiple of 16 up to 512, B >= 1, T >= 1" in L.edgl_last_error(), bad
        assert call(dt=7) == -2 and b"dtype 7" in L.edgl_last_error()
    for arg in ("xp", "R", "bR", "h", "pack"):
        assert fwd(**{arg: None}) == -4 and b"edgl_lstm_seq_fwd: null" in L.edgl_last_error(), arg
    for arg in ("dh", "R", "sv", "dxp", "pack"):
        assert bwd(**{arg: None}) == -4 and b"edgl_lstm_seq_bwd: null" in L.edgl_last_error(), arg
    # the forward pack: [C/16 tiles][C/32 k-blocks][4 gates] bf16 fragments of 1 KiB = 4 C^2 elements (the backward's is as large)
    assert L.edgl_lstm_seq_pack_bytes(512, 1) == 4 * 512 * 512 * 2 and L.edgl_lstm_seq_pack_bytes(144, 1) == 4 * 144 * 160 * 2
    assert all(L.edgl_lstm_seq_pack_bytes(C, dt) == -1 for C, dt in ((24, 0), (528, 1), (0, 0), (64, 7)))


def test_layer_draws_eight_orthogonal_blocks_and_zero_biases():
    from easydgl_amd.module import sequential as S
    m = S.LSTM(64, gen=torch.Generator().manual_seed(1))
    assert m.w_kernel.shape == m.r_kernel.shape == (64, 256) and m.w_bias.shape == m.r_bias.shape == (256,)
    mats = [k.detach().numpy()[:, g * 64:(g + 1) * 64] for k in (m.w_kernel, m.r_kernel) for g in range(4)]
    assert all(np.abs(a.T @ a - np.eye(64)).max() < 1e-5 for a in mats)
    assert all(not np.allclose(mats[i], mats[j]) for i in range(8) for j in range(i))
    assert not m.w_bias.any() and not m.r_bias.any()
    with pytest.raises(ValueError, match="multiple of 16"):
        S.LSTM(24)


def test_model_names_shapes_and_round_trip():
    from easydgl_amd.module import sequential as S
    m = _model(rnn_cell="lstm")
    m._shadow = None        # (not finalised: no device copies to refresh)
    assert all(isinstance(l, S.LSTM) for l in m.layers) and all(isinstance(l, S.GRU) for l in _model().layers)
    shapes, vals = LR.shapes(50, 32, 2), m.tf_values()
    assert {k: v.shape for k, v in vals.items()} == shapes and len(shapes) == 2 + 2 * 16
    new = SR.init_from_shapes(shapes, np.random.default_rng(3))
    m.load_tf_variables(new)
    back = m.tf_values()
    assert all(np.array_equal(back[k], new[k].astype(np.float32)) for k in shapes)


def test_refusals_name_the_flag():
    from easydgl_amd import train
    with pytest.raises(ValueError, match="--rnn_cell"):
        _model(rnn_cell="rnn")
    with pytest.raises(ValueError, match="--rnn_cell lstm with --model SASREC"):
        train.run(SimpleNamespace(model="SASREC", seed=1, rnn_cell="lstm"))
    argv = ["--train", "a", "--valid", "a", "--test", "a", "--model", "GRU4REC", "--num_items", "9"]
    assert train.args(argv).rnn_cell == "gru" and train.args(argv + ["--rnn_cell", "lstm"]).rnn_cell == "lstm"
