"""FP8 two-stage retrieval, the parts that need no GPU: the entry points refuse bad arguments before any launch, the
model names the missing call, the driver refuses the flag beside the protocols that draw no list."""
from types import SimpleNamespace

import pytest

ONE = 16      # any non-null, 16-byte aligned address: the checks below fail before a pointer is dereferenced


def _topk(L, rows=ONE, C=128, K=50, i0=0, i1=5000, I=5000):
    return L.edgl_score_topk_fp8(rows, ONE, ONE, ONE, ONE, None, 0, 4, C, I, i0, i1, K, ONE, ONE, ONE, None)


@pytest.mark.parametrize("kw,code,text", [(dict(rows=None), -4, b"null"), (dict(C=48), -1, b"power of two"), (dict(K=1025), -1, b"1024"),
                                          (dict(i0=4), -1, b"i0 % 8"), (dict(i0=4960, K=50), -1, b"fewer than K"),
                                          (dict(i1=300000, I=300000), -1, b"262144")])
def test_score_topk_fp8_refuses_before_any_launch(kw, code, text):
    from easydgl_amd import _lib
    L = _lib.lib
    assert _topk(L, **kw) == code and text in L.edgl_last_error(), L.edgl_last_error()


def test_queries_and_quantiser_checks():
    from easydgl_amd import _lib
    L = _lib.lib
    assert L.edgl_score_topk_fp8_supported(512, 256, 262144, 201, 200) == 1 and L.edgl_score_topk_fp8_workspace(512, 256, 262144, 201, 200) > 0
    for bad in [(4, 48, 5000, 0, 50), (4, 128, 5000, 0, 1025), (4, 128, 40, 0, 50), (4, 128, 300000, 0, 50), (0, 128, 5000, 0, 50)]:
        assert L.edgl_score_topk_fp8_supported(*bad) == 0 and L.edgl_score_topk_fp8_workspace(*bad) < 0, bad
    assert L.edgl_rows_to_fp8(None, 4, 64, 0, ONE, ONE, None, None) == -4
    assert L.edgl_rows_to_fp8(ONE, 4, 48, 0, ONE, ONE, None, None) == -1 and b"power of two" in L.edgl_last_error()
    assert L.edgl_rows_to_fp8(ONE, 4, 64, 7, ONE, ONE, None, None) == -2


def test_retrieve_without_an_image_names_the_call():
    from easydgl_amd.model.base import Sequential
    with pytest.raises(RuntimeError, match="quantize_items"):
        Sequential.retrieve(SimpleNamespace(), {}, 10)


def test_driver_refuses_the_short_list_beside_the_listless_protocols(capsys):
    from easydgl_amd import train
    base = ["--train", "a", "--valid", "b", "--test", "c", "--model", "TiSASREC", "--num_items", "100"]
    assert train.args(base).eval_fp8_shortlist == 0 and train.args(base + ["--eval_fp8_shortlist", "200"]).eval_fp8_shortlist == 200
    for other in (["--eval_by_rank"], ["--eval_negatives", "50"]):
        with pytest.raises(SystemExit):
            train.args(base + ["--eval_fp8_shortlist", "200"] + other)
        err = capsys.readouterr().err
        assert "--eval_fp8_shortlist" in err and other[0] in err
