"""The host side of the scoring / compaction / CE / top-K entry points answers what it answered at the commit recorded in
tests/golden/score_host_parent.json (tests/golden/make_score_host.py): the workspace sizes, slab offsets and chunk counts that
engines cache, with the strip kernels on and off, and the return code and edgl_last_error text of every rejected call.  No call
here reaches a launch, so no GPU is needed."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("_make_score_host", os.path.join(HERE, "golden", "make_score_host.py"))
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def recorded():
    with open(gen.PATH) as f:
        return json.load(f)


@pytest.mark.parametrize("mode", sorted(gen.MODES))
def test_plan_queries_answer_as_recorded(recorded, mode):
    got, want = gen.plans_in_child(mode), recorded["plans"][mode]      # a fresh process: the switches are latched once
    for kind in ("chunks", "nparts", "plan"):
        assert set(got[kind]) == set(want[kind]), kind
        diff = {k: (want[kind][k], got[kind][k]) for k in want[kind] if got[kind][k] != want[kind][k]}
        assert not diff, (kind, len(diff), sorted(diff.items())[:5])
    assert len(want["plan"]) == 8 * 5 * 8 * 2        # R x C x (I, n_items) x dtype
    # the switches reached the child: the strip kernels plan their own flash workspace at bf16 C = 128 / 256 / 512 and nowhere else
    other = recorded["plans"]["strips_off" if mode == "default" else "default"]["plan"]
    differ = {k.split(",")[1] + "/" + k.split(",")[4] for k in other if got["plan"][k] != other[k]}
    assert differ and differ <= {"128/1", "256/1", "512/1"}, differ


def test_rejected_calls_answer_as_recorded(recorded):
    from easydgl_amd import _lib
    want = recorded["rejections"]
    assert [w[:2] for w in want] == [[n, lab] for n, lab, _ in gen.rejection_cases()]
    assert all(w[2] != 0 for w in want)              # the file holds rejected calls only: nothing replayed here launches
    got = gen.rejections(_lib.lib)
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, diff[:5]
    assert {w[0] for w in want} == set(gen.SPECS) and len(want) > 200
