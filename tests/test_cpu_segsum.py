"""Host-side queries of the deterministic item-table scatter (csrc/k_segsum.hip): callable without a GPU."""
import pytest


def _bits(x: int) -> int:
    return int(x).bit_length()


@pytest.mark.parametrize("I", [2, 256, 257, 65536, 65537, 1000001])
def test_passes_are_the_bytes_of_the_largest_key(I):
    from easydgl_amd import _lib
    want = -(-_bits(I - 1) // 8)
    assert _lib.lib.edgl_segsum_passes(I) == want
    assert {2: 1, 256: 1, 257: 2, 65536: 2, 65537: 3, 1000001: 3}[I] == want


def test_plan_bytes_cover_the_plan_and_grow_with_n():
    from easydgl_amd import _lib
    L = _lib.lib
    last = 0
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 51712, 70001):
        for I in (2, 257, 20001, 1000001):
            b = L.edgl_segsum_plan_bytes(n, I)
            n4 = (n + 3) // 4 * 4
            # the caller-visible front (include/easydgl_hip.h): header, perm, seg_key, seg_start with its closing entry
            assert b >= 4 * (4 + 2 * n4 + n + 1), (n, I, b)
            assert b >= 4 * (n + n + n + 1)
        b = L.edgl_segsum_plan_bytes(n, 20001)
        assert b > 0 and b >= last, (n, b, last)
        last = b
    assert L.edgl_segsum_plan_bytes(0, 10) == -1 and L.edgl_segsum_plan_bytes(10, 1) == -1
    assert L.edgl_segsum_passes(1) == -1


def test_entry_points_reject_bad_arguments_before_any_launch():
    from easydgl_amd import _lib
    L, one = _lib.lib, 16      # `one`: any aligned non-null address — the checks fail before a pointer is dereferenced
    assert L.edgl_segsum_plan(None, 8, None, 10, 0, 10, one, None) == -4
    assert L.edgl_segsum_plan(one, 8, None, 10, 4, 4, one, None) == -1            # empty range
    assert L.edgl_segsum_plan(one, 8, None, 10, 0, 10, 8, None) == -1             # plan buffer not 16-byte aligned
    rc = L.edgl_encode_bwd_add_det(one, one, one, None, None, 2, 4, 32, 4, 10, 0.0, None, 0, one, one, one, one, 0, None, 0, None)
    assert rc == -4 and b"plan" in L.edgl_last_error()
    rc = L.edgl_score_flash_label_term_det(one, one, one, None, 8, 128, 10, 0, 10, None, one, one, None, 1, None)
    assert rc == -4


def test_driver_refuses_the_mode_for_models_it_does_not_cover(tmp_path):
    """--deterministic holds for EasyDGL only (the regressive models keep f32-atomic scatters): the driver raises, it never
    silently runs without the promise."""
    import numpy as np
    from easydgl_amd import train as TR
    ids = np.ones((4, 11), dtype=np.int64)
    np.savez(tmp_path / "d.npz", seqs_i=ids, seqs_t=np.zeros((4, 11), dtype=np.float32))
    f = str(tmp_path / "d.npz")
    with pytest.raises(ValueError, match="deterministic"):
        TR.main(["--model", "TGAT", "--train", f, "--valid", f, "--test", f, "--num_items", "10", "--seqslen", "10", "--deterministic"])
