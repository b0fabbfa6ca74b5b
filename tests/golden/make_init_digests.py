"""Generates tests/golden/models/init_digests.json — sha256 digests of the INITIAL parameters of the four models.

A model draws its initial values from one seeded generator, in the order of its module constructors and then (channel-padded
widths) of its variable table; a refactor of the model layer must not move a single draw.  The file records what THIS project's
code produced at the commit named in it: for each of EasyDGL / CTSMA / TGAT / TiSASREC at (num_units, num_heads) = (32, 2)
(unpadded), (20, 2) (head dim 10 stored as 16) and (48, 1) (48 stored as 64) a sha256 over named_parameters() (name + bytes), for
EasyDGL also over the time code's `scale`.  tests/test_cpu_models.py rebuilds the models and compares.  Regenerate only on purpose
(an intended change of an initialiser), on a clean checkout:

    python tests/golden/make_init_digests.py
"""
import hashlib
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import easydgl_oracle as O  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "models", "init_digests.json")
MODELS = ("EasyDGL", "CTSMA", "TGAT", "TiSASREC")
WIDTHS = ((32, 2), (20, 2), (48, 1))      # (num_units, num_heads): unpadded, 10 -> 16, 48 -> 64
FIXED = dict(num_blocks=2, seqslen=10, num_items=50, num_events=4, masklen=3, timelen=16, seed=7)


def flags(model, num_units, num_heads):
    f = FIXED
    return SimpleNamespace(model=model, num_items=f["num_items"], num_units=num_units, num_heads=num_heads, num_blocks=f["num_blocks"],
                           seqslen=f["seqslen"], masklen=f["masklen"], timelen=f["timelen"], seed=f["seed"], time_scale=86400.0,
                           learning_rate=1e-3, l2_reg=1e-4, ct_reg=1e-3, hidden_dropout_rate=0.1, attention_probs_dropout_rate=0.1,
                           mark_table=O.synthetic_mark_table(f["num_items"], f["num_events"], multi_hot=True), compute_dtype="f32",
                           num_train_steps=None, num_warmup_steps=None)


def digest(named_tensors):
    h = hashlib.sha256()
    for name, t in named_tensors:
        a = np.ascontiguousarray(t.detach().cpu().numpy())
        h.update(name.encode() + b"\0" + str(a.dtype).encode() + b"\0" + repr(a.shape).encode() + b"\0")
        h.update(a.tobytes())
    return h.hexdigest()


def model_digests(model, num_units, num_heads):
    import easydgl_amd
    m = easydgl_amd.ranking(flags(model, num_units, num_heads))
    out = {"parameters": digest(m.named_parameters())}
    if model == "EasyDGL":
        out["tcoding.scale"] = digest([("tcoding.scale", m.tcoding.scale)])
    return out


def key(model, num_units, num_heads):
    return f"{model}/{num_units}x{num_heads}"


def main():
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    dirty = subprocess.run(["git", "status", "--porcelain", "--", "easydgl_amd"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    out = {"commit": commit + ("+dirty" if dirty else ""), "config": FIXED, "digests": {}}
    for model in MODELS:
        for C, h in WIDTHS:
            out["digests"][key(model, C, h)] = model_digests(model, C, h)
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(PATH, len(out["digests"]), "models at", out["commit"])


if __name__ == "__main__":
    main()
