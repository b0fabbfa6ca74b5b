"""bf16 bounds of the interval attention kernels (edgl_tiattn_*) per tensor, from MEASURED errors.

Input: profiles/tiattn_parity_errors.json — the worst (relative L2, max-abs-error / max-abs-reference) per tensor over every case
of tests/test_gpu_tiattn.py (default and ordered forms) against the float64 reference tests/_tiattn_ref.py, dumped on the GPU with
EDGL_TEST_DUMP (tol_tiattn.json).
Output: tests/golden/tiattn_bf16_bounds.json — per tensor, per component: 2 x the measured maximum (rounded up to two digits; the
factor is the margin of tests/_util.py regressive_bf16_bounds and covers the order of the bin atomics), capped by what the project
accepts for a kernel without a ReLU: 3e-2 max-norm on the forward tensors (out, wbuf), GRAD_TOL["bf16"] = (2e-2 relative L2, 5e-2
max-norm) on the gradients; the forward tensors take the same 2e-2 on their relative L2.  A tensor whose MEASURED error is above
its cap is listed under over_cap and keeps the cap: the test then fails on it.  Nothing is listed for the f32 path.
        python tests/golden/make_tiattn_bounds.py"""
import json
import math
import os

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CAPS = {"out": (2e-2, 3e-2), "wbuf": (2e-2, 3e-2),
        **{k: (2e-2, 5e-2) for k in ("d_q", "d_k", "d_v", "d_ktime", "d_vtime")}}      # (relative L2, max-norm)
FACTOR = 2.0


def up2(x: float) -> float:
    """round up to two significant digits"""
    e = math.floor(math.log10(x)) - 1
    return round(math.ceil(x / 10 ** e) * 10 ** e, 12)


def main():
    src = json.load(open(os.path.join(ROOT, "profiles", "tiattn_parity_errors.json")))
    out = {"source": "profiles/tiattn_parity_errors.json",
           "rule": f"per component: min(cap, {FACTOR} x measured maximum); caps (relative L2, max-norm): {CAPS}",
           "bounds": {}, "measured": {}, "over_cap": {}}
    for key, (l2, mx) in src.items():
        mode, name = key.split(":", 1)
        if mode == "bf16":
            out["measured"][name] = [l2, mx]
    for name, cap in CAPS.items():
        m = out["measured"][name]
        if m[0] > cap[0] or m[1] > cap[1]:
            out["over_cap"][name] = m
        out["bounds"][name] = [min(cap[i], up2(FACTOR * m[i])) for i in range(2)]
    json.dump(out, open(os.path.join(HERE, "tiattn_bf16_bounds.json"), "w"), indent=1, sort_keys=True)
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
