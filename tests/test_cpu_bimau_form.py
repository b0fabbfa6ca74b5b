"""edgl_bimau_form and the size queries of the two BiMAU kernel families (host functions: no GPU needed)."""
import pytest

F32, BF16 = 0, 1
STREAM = 16


def lib():
    from easydgl_amd import _lib
    return _lib


@pytest.mark.parametrize("T,C,H,dt", [(101, 128, 8, BF16), (201, 256, 8, BF16), (128, 128, 1, BF16), (112, 64, 1, F32),
                                      (208, 32, 2, F32), (208, 64, 2, BF16), (128, 64, 2, F32), (64, 128, 1, F32)])
def test_in_register_shapes_keep_their_kernels(T, C, H, dt):
    L = lib()
    from easydgl_amd import ops
    assert L.MAU_STREAM == STREAM == ops.MAU_STREAM
    assert L.lib.edgl_bimau_form(T, C, H, dt, 0) == 0
    assert L.lib.edgl_bimau_form(T, C, H, dt, L.MAU_NO_SKIP) == 0
    assert L.lib.edgl_bimau_form(T, C, H, dt, STREAM) == 1          # the hint forces the key-streamed family
    assert L.lib.edgl_bimau_form(T, C, H, dt, STREAM | 3) == 1


@pytest.mark.parametrize("T,C,H,dt", [(209, 32, 2, F32), (209, 32, 2, BF16), (150, 64, 2, F32), (129, 128, 2, BF16), (113, 64, 1, F32),
                                      (65, 256, 2, F32), (1024, 32, 2, F32), (1024, 32, 2, BF16), (129, 256, 2, BF16), (209, 64, 2, BF16)])
def test_shapes_beyond_the_in_register_bounds_are_streamed(T, C, H, dt):
    assert lib().lib.edgl_bimau_form(T, C, H, dt, 0) == 1


def test_unsupported_shapes_are_negative():
    L = lib().lib
    assert L.edgl_bimau_form(1025, 32, 2, BF16, 0) < 0
    assert L.edgl_bimau_form(1025, 32, 2, F32, STREAM) < 0
    assert L.edgl_bimau_form(30, 48, 1, F32, 0) < 0          # head dim 48
    assert L.edgl_bimau_form(30, 96, 2, BF16, STREAM) < 0
    assert L.edgl_bimau_form(30, 33, 2, F32, 0) < 0          # C % H != 0
    assert L.edgl_bimau_form(0, 32, 2, F32, 0) < 0
    assert L.edgl_bimau_form(30, 32, 2, 7, 0) < 0            # dtype code 7


# (B, T, C, H, dtype) -> (saved bytes, workspace bytes at E = 16, at E = 5): values of the library BEFORE the key-streamed family
# existed, taken from a build of that commit — a shape of the in-register kernels must keep exactly these
PARENT_SIZES = {
    (4, 101, 128, 8, BF16): (310272, 8131328, 2994944),
    (2, 201, 256, 8, BF16): (411648, 28592896, 9669376),
    (3, 128, 128, 1, BF16): (122880, 17394432, 17329664),
    (2, 112, 64, 1, F32): (71680, 8856832, 8827136),
    (2, 31, 64, 2, F32): (23808, 27590144, 8666624),
}


@pytest.mark.parametrize("shape", sorted(PARENT_SIZES))
def test_size_queries_of_in_register_shapes_are_unchanged(shape):
    L = lib().lib
    B, T, C, H, dt = shape
    saved, ws16, ws5 = PARENT_SIZES[shape]
    assert L.edgl_bimau_saved_bytes(B, T, C, H, dt) == saved
    assert L.edgl_bimau_saved_bytes_ex(B, T, C, H, dt, 0) == saved
    assert L.edgl_bimau_bwd_workspace(B, T, C, H, 16, dt) == ws16
    assert L.edgl_bimau_bwd_workspace(B, T, C, H, 5, dt) == ws5
    assert L.edgl_bimau_bwd_workspace_ex(B, T, C, H, 16, dt, 0) == ws16


def _form0_saved(B, T, C, H, es):
    """[H*B*T, dh] activations, 256-byte aligned, then z [H*B*T, 16] f32 (csrc/bimau_common.h saved_layout)"""
    R = B * H * T
    return ((R * (C // H) * es + 255) & ~255) + R * 16 * 4


@pytest.mark.parametrize("B,T,C,H,dt,flags", [(2, 209, 32, 2, BF16, 0), (3, 257, 32, 2, F32, 0), (2, 201, 512, 8, BF16, 0),
                                              (2, 1024, 32, 2, F32, 0), (2, 101, 128, 8, BF16, STREAM), (2, 31, 64, 2, F32, STREAM)])
def test_streamed_shapes_add_the_row_statistics(B, T, C, H, dt, flags):
    L = lib().lib
    R = B * H * T
    base = _form0_saved(B, T, C, H, 2 if dt == BF16 else 4)
    got = L.edgl_bimau_saved_bytes_ex(B, T, C, H, dt, flags)
    assert got >= base + R * 2 * 4                        # (row maximum, 1 / sum) f32 per row
    if flags == 0:
        assert L.edgl_bimau_saved_bytes(B, T, C, H, dt) == got      # the plain query knows the form of the shape
        assert L.edgl_bimau_bwd_workspace(B, T, C, H, 4, dt) == L.edgl_bimau_bwd_workspace_ex(B, T, C, H, 4, dt, 0)
    else:
        assert got > L.edgl_bimau_saved_bytes(B, T, C, H, dt)
    # the streamed sweep 1 leaves one row of dscaling partials per (job, query tile) instead of one per job
    nt = (T + 15) // 16
    if flags:
        assert L.edgl_bimau_bwd_workspace_ex(B, T, C, H, 4, dt, flags) >= L.edgl_bimau_bwd_workspace(B, T, C, H, 4, dt) + B * H * (nt - 1) * 16 * 4 - 256
    assert L.edgl_bimau_bwd_workspace_ex(B, T, C, H, 4, dt, flags) > 0
    assert L.edgl_bimau_saved_bytes_ex(B, T, 33, 2, dt, flags) == -1
