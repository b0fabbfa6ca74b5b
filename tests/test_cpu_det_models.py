"""Host side of the deterministic mode of CTSMA / TGAT / TiSASRec: the size query, the argument checks of the new
entry points (they fail before any launch, so no GPU is needed) and where the models read the flag."""
from types import SimpleNamespace

NULL, SHAPE, DTYPE = -4, -1, -2


def test_codes_are_the_librarys():
    from easydgl_amd import _lib
    L, one = _lib.lib, 16
    assert L.edgl_segsum_plan(None, 8, None, 10, 0, 10, one, None) == NULL
    assert L.edgl_segsum_plan(one, 0, None, 10, 0, 10, one, None) == SHAPE
    assert L.edgl_embedding_bwd(one, 8, one, 4, 32, 1, 1.0, one, 7, None) == DTYPE


def test_tiattn_det_workspace_sizes():
    from easydgl_amd import _lib
    L = _lib.lib
    for H, dh, timelen in ((1, 16, 1), (2, 16, 8), (2, 64, 256), (8, 16, 256), (1, 128, 64), (4, 32, 50)):
        n = L.edgl_tiattn_det_workspace(H, dh, timelen)
        # two tables, one slab per row split, every table row the kernels can be handed (timelen + 1)
        assert n > 0 and n % (2 * (timelen + 1) * H * dh) == 0, (H, dh, timelen, n)
        assert n // (2 * (timelen + 1) * H * dh) >= 2
    for bad in ((0, 16, 8), (2, 24, 8), (2, 256, 8), (2, 16, 0), (2, 16, 257), (-1, 16, 8)):
        assert L.edgl_tiattn_det_workspace(*bad) == -1, bad


def test_embed_pos_bwd_det_rejects_bad_arguments_before_any_launch():
    from easydgl_amd import _lib
    L, one = _lib.lib, 16

    def call(ids=one, dx0=one, B=2, T=4, C=32, I=10, d_item=one, d_pos=one, c_true=0, plan=one, dtype=0):
        return L.edgl_embed_pos_bwd_det(ids, dx0, B, T, C, I, 0.0, None, 0, d_item, d_pos, c_true, plan, dtype, None)

    assert call(ids=None) == NULL and call(dx0=None) == NULL and call(d_item=None) == NULL
    assert call(plan=None) == NULL and b"edgl_embed_pos_bwd_det" in L.edgl_last_error()
    assert call(B=0) == SHAPE and call(T=0) == SHAPE and call(C=30) == SHAPE and call(C=516) == SHAPE and call(I=1) == SHAPE
    assert call(c_true=33) == SHAPE
    assert call(plan=8) == SHAPE           # not 16-byte aligned
    assert call(dtype=5) == DTYPE


def test_embedding_bwd_det_rejects_bad_arguments_before_any_launch():
    from easydgl_amd import _lib
    L, one = _lib.lib, 16

    def call(ids=one, n=8, d_out=one, rows=4, C=32, zero_pad=1, d_table=one, plan=one, dtype=1):
        return L.edgl_embedding_bwd_det(ids, n, d_out, rows, C, zero_pad, 1.0, d_table, plan, dtype, None)

    assert call(ids=None) == NULL and call(d_out=None) == NULL and call(d_table=None) == NULL and call(plan=None) == NULL
    assert call(n=0) == SHAPE and call(rows=0) == SHAPE and call(C=6) == SHAPE and call(C=1024) == SHAPE
    assert call(plan=24) == SHAPE
    assert call(dtype=-1) == DTYPE


def test_tiattn_bwd_det_rejects_bad_arguments_before_any_launch():
    from easydgl_amd import _lib
    L, one = _lib.lib, 16

    def call(q=one, ws=one, tab_rows=8, B=2, T=8, H=2, dh=16, timelen=8, ld=32, d_kt=one, rate=0.0, dtype=0):
        return L.edgl_tiattn_bwd_det(q, ld, one, 64, one, 64, one, one, one, one, tab_rows, one, 32, one, one, B, T, H, dh, 0.25, 1.0,
                                     timelen, rate, None, 0, one, 32, one, 64, one, 64, one, d_kt, one, ws,
                                     _lib.TATTN_CAUSAL | _lib.TATTN_ORDERED, dtype, None)

    assert call(ws=None) == NULL and b"workspace" in L.edgl_last_error()
    assert call(q=None) == NULL and call(d_kt=None) == NULL
    assert call(rate=0.1) == NULL          # dropout without an rng state
    assert call(dh=24) == SHAPE and call(T=300) == SHAPE and call(timelen=300) == SHAPE and call(tab_rows=10) == SHAPE
    assert call(ld=30) == SHAPE and call(ws=8) == SHAPE and call(d_kt=8) == SHAPE
    assert call(dtype=3) == DTYPE
    assert _lib.TATTN_ORDERED == 2 and _lib.TATTN_ORDERED & _lib.TATTN_CAUSAL == 0


def test_models_read_the_flag_in_one_place():
    """Sequential.__init__ reads FLAGS.deterministic for all four models; TiSASRec hands it to its attention units."""
    import inspect
    from easydgl_amd.model import base, ctsma, easydgl, tgat, tisasrec
    assert "FLAGS, \"deterministic\"" in inspect.getsource(base.Sequential.__init__)
    for mod in (ctsma, easydgl, tgat, tisasrec):
        assert "FLAGS, \"deterministic\"" not in inspect.getsource(mod)
    F = SimpleNamespace(model="TiSASREC", num_items=20, num_units=32, num_heads=2, num_blocks=1, seqslen=8, timelen=16, time_scale=1.0,
                        learning_rate=1e-3, deterministic=True)
    from easydgl_amd.util import ranking
    m = ranking(F)
    assert m.deterministic is True
    assert all(b.attention.deterministic is False for b in m.layers)      # finalize() hands it over, with time_scale and timelen
    assert "blk.attention.deterministic = self.deterministic" in inspect.getsource(tisasrec.TiSASRec.finalize)
