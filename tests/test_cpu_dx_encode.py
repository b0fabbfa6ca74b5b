"""Host side of the fused QKVT dX GEMM + embedding backward (edgl_dx_encode_bwd_label): callable without a GPU."""


def test_query_is_a_function_of_the_shape_alone():
    from easydgl_amd import _lib
    q = _lib.lib.edgl_dx_encode_supported
    assert [q(B, 101, 128, _lib.BF16) for B in (120, 128, 250, 512, 2048)] == [1, 1, 1, 1, 1]
    assert [q(B, 101, 128, _lib.BF16) for B in (4, 129, 0, 2049)] == [0, 0, 0, 0]      # padded samples > B / 8; more than 16 chunks
    assert q(128, 101, 128, _lib.F32) == 0 and q(128, 101, 256, _lib.BF16) == 0 and q(128, 0, 128, _lib.BF16) == 0


def test_entry_point_rejects_bad_arguments_before_any_launch():
    from easydgl_amd import _lib
    L, one = _lib.lib, 16      # `one`: any aligned non-null address — the checks fail before a pointer is dereferenced

    def call(dqkvt=one, W=one, B=128, T=17, C=128, lab_rows=one, add2=one, dtype=_lib.BF16, lda=512, rate=0.0):
        return L.edgl_dx_encode_bwd_label(dqkvt, W, lda, 4 * C, None, one, one, one, add2, B, T, C, 16, 300, rate, None, 1, one, one, one,
                                          one, 0, lab_rows, one, one, None, 15, one, dtype, None)
    assert call(dqkvt=None) == -4 and call(W=None) == -4 and b"edgl_dx_encode_bwd_label" in L.edgl_last_error()
    assert call(lab_rows=None) == -4           # the label operands are not optional
    assert call(add2=None) == -4               # add1 without add2
    assert call(rate=0.1) == -4                # dropout without an RNG state
    assert call(dtype=_lib.F32) == -2          # f32 keeps the unfused pair
    assert call(C=256) == -1 and call(B=4) == -1 and call(B=129) == -1
    assert call(lda=500) == -1                 # row stride below 4C
    assert call(dqkvt=8) == -1                 # GEMM operand not 16-byte aligned
