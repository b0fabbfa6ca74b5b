"""The host side of the TPP / optimizer / reduction entry points (k_tpp.hip, k_optim.hip, k_reduce.hip) answers what it answered at
the commit recorded in tests/golden/misc_host_parent.json (tests/golden/make_misc_host.py): the workspace sizes engines cache, and
the return code and edgl_last_error text of every rejected call.  No call here reaches a launch, so no GPU is needed."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("_make_misc_host", os.path.join(HERE, "golden", "make_misc_host.py"))
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def recorded():
    with open(gen.PATH) as f:
        return json.load(f)


def test_size_queries_answer_as_recorded(recorded):
    from easydgl_amd import _lib
    got, want = gen.sizes(_lib.lib), recorded["sizes"]
    assert got == want, [(k, a, want[k][a], got[k][a]) for k in want if isinstance(want[k], dict) for a in want[k] if got[k][a] != want[k][a]][:5]
    assert len(want["tpp_rows_workspace"]) == 5 * 4 * 9 and len(want["tpp_prep_bytes"]) == 4 * 6 * 5 and len(want["adam_l2_parts"]) == 10
    assert want["tpp_rows_workspace"]["0,3,4"] == -1 and want["tpp_prep_bytes"]["6,-1,4"] == -1 and want["adam_l2_parts"]["0"] == -1


def test_rejected_calls_answer_as_recorded(recorded):
    from easydgl_amd import _lib
    want = recorded["rejections"]
    assert [w[:2] for w in want] == [[n, lab] for n, lab, _ in gen.rejection_cases()]
    assert all(w[2] != 0 for w in want)              # the file holds rejected calls only: nothing replayed here launches
    got = gen.rejections(_lib.lib)
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, diff[:5]
    assert {w[0] for w in want} == set(gen.SPECS) and len(want) > 120
    # edgl_tpp_fwd_bwd_ex reports itself under the name of the entry point the engine calls
    assert all(w[3].startswith("edgl_tpp_fwd_bwd: ") for w in want if w[0] == "edgl_tpp_fwd_bwd_ex")


def test_deferred_mode_on_and_abort_launch_nothing(recorded):
    from easydgl_amd import _lib
    assert gen.queue(_lib.lib) == recorded["queue"] == [0, 0]


def test_adam_apply_ex_refuses_slabs_without_a_slab_count(recorded):
    """Not in the parent's file: there the call passed validation and the vector path read slab min(k, nslab - 1) = -1."""
    from easydgl_amd import _lib
    shape_rc = next(w[2] for w in recorded["rejections"] if w[0] == "edgl_adam_apply_ex" and w[1] == "nslab=-1")
    for ov in gen.NSLAB_ZERO:
        rc, err = gen.call(_lib.lib, "edgl_adam_apply_ex", gen.call_args("edgl_adam_apply_ex", ov))
        assert rc == shape_rc      # EDGL_ERR_SHAPE, as for the other bad slab ranges
        assert err == "edgl_adam_apply_ex: slabs given with nslab = 0 (>= 1)"
