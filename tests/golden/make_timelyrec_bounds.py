"""bf16 gradient bounds of TimelyREC per tensor class, from MEASURED errors.

Input: profiles/timelyrec_parity_errors.json — the worst (relative L2, max-abs-error / max-abs-reference) per tensor over the cases
of tests/test_gpu_timelyrec.py::test_forward_loss_and_gradients against the fp64 restatement (tests/_timelyrec_ref.py), dumped on
the GPU with EDGL_TEST_DUMP (tol_timelyrec.json).
Output: tests/golden/timelyrec_bf16_bounds.json — per tensor class, per component: tests/_util.py's GRAD_TOL["bf16"] where the
class's measured maximum meets it, else 2 x that maximum (rounded up to two digits; the factor covers draw-to-draw variation).  A
class that is not listed keeps GRAD_TOL["bf16"]; nothing is listed for the f32 path.  The relative-L2 bound is capped at CAP (the cap
tests/_util.py regressive_bf16_bounds puts on its classes); a class whose MEASURED relative L2 is above CAP is NOT listed (the test
then fails on it: DESIGN 4.18 names the operand whose rounding causes it).  The ReLU-gated Inner tensors
keep relu_flip_err's own condition; the K bias (true gradient zero) has its own check in the test and is not dumped.
        python tests/golden/make_timelyrec_bounds.py"""
import json
import math
import os

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
DEFAULT = (2e-2, 5e-2)      # tests/_util.py GRAD_TOL["bf16"]
FACTOR = 2.0
CAP = 8e-2                  # the cap tests/_util.py regressive_bf16_bounds uses


def tensor_class(name: str) -> str:
    """Class of a gradient tensor: the branch it belongs to (item / position / calendar tables, user branch attention and
    feed-forward, slot encoder, head) and its kind (kernel / bias / LayerNorm)."""
    if "/Inner/" in name:
        return "ffn_inner"
    if name.endswith("te_weight"):
        return "te_weight"
    if name.endswith("output_bias"):
        return "output_bias"
    if name.endswith("lookup_table"):
        return "calendar_table" if any(f"/{g}_embs/" in name for g in ("month", "day", "weekday", "hour")) else "table"
    if "/mate/" in name:
        return "mate_kernel"
    part = "attn" if "Atttention" in name else "ffn" if "fforward" in name else "pred" if "prediction" in name else "out"
    if "LayerNorm" in name:
        return part + "_layernorm"
    return part + ("_bias" if name.endswith("bias") else "_kernel")


def up2(x: float) -> float:
    """round up to two significant digits"""
    e = math.floor(math.log10(x)) - 1
    return round(math.ceil(x / 10 ** e) * 10 ** e, 12)


def main():
    src = json.load(open(os.path.join(ROOT, "profiles", "timelyrec_parity_errors.json")))
    out = {"source": "profiles/timelyrec_parity_errors.json",
           "rule": f"per component: GRAD_TOL['bf16'] {DEFAULT} where the measured class maximum meets it, else {FACTOR} x measured; "
                   f"no class above {CAP} relative L2 is listed",
           "bounds": {}, "measured": {}, "over_cap": {}}
    for key, (l2, mx) in src.items():
        mode, name = key.split(":", 1)
        if mode != "bf16" or name.endswith("multihead_attention/dense_1/bias"):
            continue
        w = out["measured"].setdefault(tensor_class(name), [0.0, 0.0])
        w[0], w[1] = max(w[0], l2), max(w[1], mx)
    for c, (l2, mx) in out["measured"].items():
        if c == "ffn_inner" or (l2 <= DEFAULT[0] and mx <= DEFAULT[1]):
            continue
        if l2 > CAP:
            out["over_cap"][c] = [l2, mx]
            continue
        b2 = DEFAULT[0] if l2 <= DEFAULT[0] else min(up2(FACTOR * l2), CAP)      # (capped, as regressive_bf16_bounds caps its classes)
        out["bounds"][c] = [b2, DEFAULT[1] if mx <= DEFAULT[1] else up2(FACTOR * mx)]
    json.dump(out, open(os.path.join(HERE, "timelyrec_bf16_bounds.json"), "w"), indent=1, sort_keys=True)
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
