"""bf16 gradient bounds of SASREC / S2PNM per tensor class, from MEASURED errors.

Input: profiles/seq_baselines_parity_errors.json — the worst (relative L2, max-abs-error / max-abs-reference) per tensor over the
cases of tests/test_gpu_seq_baselines.py::test_forward_loss_and_gradients against the fp64 restatement
(tests/_seq_baselines_ref.py), dumped on the GPU with EDGL_TEST_DUMP (tol_seq_baselines.json).
Output: tests/golden/seq_baselines_bf16_bounds.json — per model and tensor class, per component: tests/_util.py's
GRAD_TOL["bf16"] where the class's measured maximum meets it, else 2 x that maximum (rounded up to two digits).  A class that is
not listed keeps GRAD_TOL["bf16"].  The ReLU-gated Inner tensors keep relu_flip_err's own condition and are not listed; the K bias (true
gradient zero, no relative error) has its own check in the test and is not dumped.        python tests/golden/make_seq_baselines_bounds.py"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
DEFAULT = (2e-2, 5e-2)      # tests/_util.py GRAD_TOL["bf16"]
FACTOR = 2.0


def tensor_class(name: str) -> str:
    """Class of a gradient tensor: the part of the model it belongs to (tables, GRU, attention, feed-forward, dictionary head,
    final LayerNorm) and its kind (kernel / bias / LayerNorm)."""
    if "/Inner/" in name:
        return "ffn_inner"
    if "opaque_kernel" in name:
        return "gru_bias" if "/b_" in name else "gru_kernel"
    if name.endswith("lookup_table"):
        return "table"
    if name.endswith("output_bias"):
        return "output_bias"
    low = name.lower()
    part = ("attn" if "attention" in low else "ffn" if ("feedforward" in low or "fforward" in low) else "dict" if "dictionary" in low
            else "out")
    if "LayerNorm" in name:
        return part + "_layernorm"
    return part + ("_bias" if name.endswith("bias") else "_kernel")


def up2(x: float) -> float:
    """round up to two significant digits"""
    e = math.floor(math.log10(x)) - 1
    return round(math.ceil(x / 10 ** e) * 10 ** e, 12)


def main():
    src = json.load(open(os.path.join(ROOT, "profiles", "seq_baselines_parity_errors.json")))
    out = {"source": "profiles/seq_baselines_parity_errors.json",
           "rule": f"per component: GRAD_TOL['bf16'] {DEFAULT} where the measured class maximum meets it, else {FACTOR} x measured",
           "bounds": {}, "measured": {}}
    for key, (l2, mx) in src.items():
        kind, mode, name = key.split(":", 2)
        if mode != "bf16" or name.endswith("multihead_attention/dense_1/bias"):
            continue
        w = out["measured"].setdefault(kind, {}).setdefault(tensor_class(name), [0.0, 0.0])
        w[0], w[1] = max(w[0], l2), max(w[1], mx)
    for kind, classes in out["measured"].items():
        for c, (l2, mx) in classes.items():
            if c == "ffn_inner" or (l2 <= DEFAULT[0] and mx <= DEFAULT[1]):
                continue
            out["bounds"].setdefault(kind, {})[c] = [DEFAULT[0] if l2 <= DEFAULT[0] else up2(FACTOR * l2),
                                                     DEFAULT[1] if mx <= DEFAULT[1] else up2(FACTOR * mx)]
    json.dump(out, open(os.path.join(HERE, "seq_baselines_bf16_bounds.json"), "w"), indent=1, sort_keys=True)
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
