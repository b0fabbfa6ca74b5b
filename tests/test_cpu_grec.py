"""GREC, the parts that need no GPU: the host-side masked batch, the factory key with its variable table, the
--dilations flag and the refusals by flag name."""
from types import SimpleNamespace

import pytest
import torch

from tests import _grec_ref as GR


def _flags(**kw):
    base = dict(model="GREC", num_items=50, num_units=32, num_heads=1, seqslen=9, masklen=2, filter_width=3, dilations="1,4,1,4",
                learning_rate=1e-3, compute_dtype="bf16")
    base.update(kw)
    return SimpleNamespace(**base)


def test_grec_mask_random_masks_the_drawn_positions_and_predicts_from_the_row_in_front():
    from easydgl_amd import data as D
    B, T, M, mask = 6, 10, 3, 50
    tokens = torch.randint(1, 50, (B, T), generator=torch.Generator().manual_seed(0))
    pos = D.draw_masked_positions(B, T, M, torch.Generator().manual_seed(1))
    feats, labels = D.grec_mask_random(tokens, mask, pos)
    assert set(feats) == {"seqs_i", "seqs_m", "masked_positions"} and torch.equal(feats["seqs_i"], tokens)
    hit = torch.zeros(B, T, dtype=torch.bool).scatter(1, feats["masked_positions"] + 1, True)
    assert torch.equal(feats["seqs_m"] != tokens, hit) and (feats["seqs_m"][hit] == mask).all()
    assert torch.equal(labels, tokens.gather(1, feats["masked_positions"] + 1))
    assert (feats["masked_positions"] >= 0).all() and (pos != 0).all()


def test_ranking_builds_grec_with_the_reference_variable_names():
    import easydgl_amd
    m = easydgl_amd.ranking(_flags())
    assert type(m).__name__ == "GREC" and m.static_engine_ok is False and m.num_items == 52 and m.mask_id == 50
    want = GR.grec_shapes(52, 32, 3, [1, 4, 1, 4])
    got = m.tf_values()
    assert {k: tuple(v.shape) for k, v in got.items()} == {k: tuple(s) for k, s in want.items()}
    assert [u.dconv1.dilation for u in m.masked] == [2, 8, 2, 8] and all(u.dconv0.causality for u in m.masked)


def test_dilations_flag_parses_and_unsupported_flags_are_refused_by_name(tmp_path):
    import easydgl_amd
    from easydgl_amd import train
    from easydgl_amd.model.grec import parse_dilations
    argv = ["--train", "a", "--valid", "a", "--test", "a", "--model", "GREC", "--num_items", "10"]
    a = train.args(argv)
    assert (a.filter_width, parse_dilations(a.dilations)) == (3, [1, 2, 2, 4])
    assert parse_dilations(train.args(argv + ["--dilations", "1,4,1,4"]).dilations) == [1, 4, 1, 4]
    for kw, word in ((dict(dilations="1,0"), "dilations"), (dict(num_units=48), "num_units"), (dict(filter_width=6), "filter_width"),
                     (dict(lazy_adam=True, train_negatives=4), "lazy_adam")):
        with pytest.raises(ValueError, match=word):
            easydgl_amd.ranking(_flags(**kw))
    for flag in ("--device_data", "--graph"):
        with pytest.raises(ValueError, match=flag):
            train.run(train.args(argv + [flag]))
