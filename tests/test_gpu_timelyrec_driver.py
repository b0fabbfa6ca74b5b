"""The training driver with --model TimelyREC: one epoch on a tiny synthetic set, once with the calendar fields in the
records and once without (derived from the timestamps); --graph and --device_data are refused."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
NUM_ITEMS, SEQSLEN = 300, 20


def _write(tmp_path, calendar):
    from easydgl_amd import data as D
    from easydgl_amd import formats as F
    ids, _ = D.synthetic_batch(NUM_ITEMS, SEQSLEN, 200, seed=3)
    rng = np.random.default_rng(5)
    ts = (1.6e9 + np.cumsum(rng.integers(600, 10 ** 6, size=ids.shape), axis=1)).astype(np.float32) * (ids != 0)
    cal = F.calendar_from_timestamps(ts, ids)

    def dump(name, lo, hi):
        recs = []
        for i in range(lo, hi):
            feats = {"seqs_i": ids[i], "seqs_t": ts[i]}
            if calendar:
                feats.update({k: a[i] for k, a in zip(F.CALENDAR_FIELDS, cal)})
            recs.append(F.encode_example(feats))
        F.write_tfrecord(str(tmp_path / name), recs)
    dump("train000.tfrec", 0, 140); dump("validation.tfrec", 140, 170); dump("test.tfrec", 170, 200)


def _argv(tmp_path, *extra):
    return ["--model", "TimelyREC", "--train", str(tmp_path / "train*.tfrec"), "--valid", str(tmp_path / "validation.tfrec"),
            "--test", str(tmp_path / "test.tfrec"), "--num_items", str(NUM_ITEMS), "--num_units", "32", "--num_heads", "2",
            "--num_blocks", "1", "--seqslen", str(SEQSLEN), "--batch_size", "64", "--num_epochs", "1", "--learning_rate", "1e-3",
            "--l2_reg", "1e-4", "--time_scale", "86400", "--window_ratio", "0.2", "--hidden_dropout_rate", "0.1",
            "--attention_probs_dropout_rate", "0.1", "--mask_seen", "--dtype", "bf16", "--ckpt_dir", str(tmp_path / "ckpt"), *extra]


@pytest.mark.parametrize("calendar", [True, False])
def test_driver_runs_one_epoch(tmp_path, calendar, caplog):
    from easydgl_amd import train as TR
    _write(tmp_path, calendar)
    with caplog.at_level("INFO"):
        res = TR.main(_argv(tmp_path))
    assert set(res) == {"H10", "H50", "H100", "N10", "N50", "N100"}
    assert all(0.0 <= v <= 1.0 and math.isfinite(v) for v in res.values())
    assert res["H10"] <= res["H50"] <= res["H100"]
    losses = [float(r.getMessage().split("Loss=")[1]) for r in caplog.records if "Loss=" in r.getMessage()]
    assert losses and all(math.isfinite(x) for x in losses)
    derived = [r for r in caplog.records if "derived from seqs_t" in r.getMessage()]
    assert len(derived) == (0 if calendar else 3)       # one line per split


@pytest.mark.parametrize("flag", ["--graph", "--device_data"])
def test_driver_refuses_graph_and_device_data(tmp_path, flag):
    from easydgl_amd import train as TR
    _write(tmp_path, True)
    with pytest.raises(ValueError, match="TimelyREC"):
        TR.main(_argv(tmp_path, flag))
