"""Generates tests/golden/misc_host_parent.json — what the HOST side of the TPP / optimizer / reduction entry points (k_tpp.hip,
k_optim.hip, k_reduce.hip) answers.

Three kinds of records, none of which reaches a kernel launch (so they need no GPU):
  sizes        edgl_tpp_workspace, edgl_tpp_rows_workspace, edgl_tpp_prep_bytes and edgl_adam_l2_parts over a small grid that includes
               non-positive arguments — engines cache these numbers.
  rejections   (return code, edgl_last_error text) of calls that fail argument validation: each required pointer null in turn, the
               shape limits, and the special cases of single entry points.  Pointers that must be non-null are the dummy address
               ADDR: every call listed here fails before it is used.
               Only add a case after reading the entry point's checks — a call that passes them would launch on that address.
               (Optional pointers — gscale, d_lam of the one-launch forms, tpp_desc, shadow, l2_part of edgl_adam_apply_ex — have no
               "null" case for that reason, and edgl_tpp_finish_parts* put no limit on B * M: only edgl_dp_counts has that case.)
  queue        return codes of edgl_reduce_defer(1) followed by edgl_reduce_defer(-1): the pair queues and launches nothing.

The file records what the library did at the commit named in it; tests/test_cpu_misc_host.py replays the same calls against the
built library and compares exactly.  Regenerate only on purpose, with the library of a clean checkout:

    python tests/golden/make_misc_host.py [commit label]
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "misc_host_parent.json")

ROWS_GRID = [(B, H, M) for B in (-1, 0, 1, 6, 128) for H in (0, 1, 3, 8) for M in (-2, 0, 1, 4, 20, 255, 256, 257, 300)]
PREP_GRID = [(B, T, M) for B in (0, 1, 6, 128) for T in (-1, 0, 1, 21, 200, 1024) for M in (0, 1, 4, 50, 256)]
L2_GRID = (-5, 0, 1, 255, 256, 257, 4099, 1048576, 1048577, 5000000000)


def sizes(lib):
    return {"tpp_workspace": lib.edgl_tpp_workspace(),
            "tpp_rows_workspace": {"%d,%d,%d" % a: lib.edgl_tpp_rows_workspace(*a) for a in ROWS_GRID},
            "tpp_prep_bytes": {"%d,%d,%d" % a: lib.edgl_tpp_prep_bytes(*a) for a in PREP_GRID},
            "adam_l2_parts": {"%d" % n: lib.edgl_adam_l2_parts(n) for n in L2_GRID}}


# ---- rejections ---------------------------------------------------------------------------------------------------------------
ADDR = 4096      # non-null and 16-byte aligned
ADDR2 = 8192     # a second buffer (edgl_adam_apply_ex: the next step's counters)
VALS = {"B": 6, "T": 21, "H": 3, "E": 16, "M": 4, "coef": 0.5, "accumulate": 0, "with_norm": 1, "nparts": 18, "n": 4099, "lr": 1e-3,
        "beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "l2": 0.0, "nseg": 0, "P": 7, "N": 33, "ld": 40, "stride_a": 0, "lo_a": 0, "hi_a": 0,
        "zero_first_a": 0, "stride_b": 0, "lo_b": 0, "hi_b": 0, "nslab": 0, "on": 3}
TPP = "lam masked_pos labels ts_raw mark_table B T H E M coef "
TPP_REQ = ["lam", "labels", "ts_raw", "mark_table", "sums", "reg_out"]
ADAM_REQ = ["param", "grad", "m", "v", "step_state"]
L2_NO_SEG = {"l2": 0.1, "nseg": 2}
SLAB_A = {"slabs_a": ADDR, "nslab": 2, "stride_a": 64, "lo_a": 0, "hi_a": 64}
SLAB_B = {"slabs_b": ADDR, "nslab": 2, "stride_b": 64, "lo_b": 0, "hi_b": 64}
# name: (arguments in ABI order, pointers that must be non-null, own cases); masked_pos is set, and optional only with M == T
SPECS = {
    "edgl_tpp_fwd": (TPP + "sums reg_out accumulate stream", TPP_REQ + ["masked_pos"], []),
    "edgl_tpp_bwd": (TPP + "sums gscale d_lam stream", ["lam", "labels", "ts_raw", "mark_table", "sums", "d_lam", "masked_pos"], []),
    "edgl_tpp_fwd_bwd": (TPP + "sums reg_out accumulate d_lam stream", TPP_REQ + ["masked_pos"],
                         [{"E": 0}, {"E": 17}, {"M": 257}, {"T": 1025}]),
    "edgl_tpp_fwd_bwd_ex": (TPP + "sums reg_out accumulate d_lam with_norm stream", TPP_REQ + ["masked_pos"],
                            [{"E": 0}, {"E": 17}, {"M": 257}, {"T": 1025}, {"E": 17, "with_norm": 0}]),
    "edgl_tpp_fwd_bwd_rows": (TPP + "sums reg_out accumulate d_lam stream", TPP_REQ + ["masked_pos"],
                              [{"E": 257}, {"E": 0}, {"B": 0}, {"H": 0}, {"M": 0}]),
    "edgl_tpp_norm": ("labels mark_table B M E sums stream", ["labels", "mark_table", "sums"], []),
    "edgl_tpp_prep": ("masked_pos labels ts_raw mark_table B T E M desc stream", ["masked_pos", "labels", "ts_raw", "mark_table", "desc"],
                      [{"E": 5}, {"E": 17}, {"M": 257}, {"M": 0}, {"T": 2049}, {"B": 0}, {"mark_table": ADDR + 4}, {"desc": ADDR + 8}]),
    "edgl_tpp_finish_parts": ("part nparts coef H tpp_desc B T M sums reg_out accumulate stream", ["part", "sums", "reg_out"],
                              [{"nparts": 0}, {"H": 0}, {"tpp_desc": ADDR, "B": 0}, {"tpp_desc": ADDR, "T": 0}, {"tpp_desc": ADDR, "M": 0}]),
    "edgl_tpp_finish_parts_n": ("part nparts coef H sums reg_out accumulate stream", ["part", "sums", "reg_out"], [{"nparts": 0}, {"H": 0}]),
    "edgl_dp_counts": ("labels mark_table B M E counts stream", ["labels", "mark_table", "counts"],
                       [{"B": 65537, "M": 1}, {"B": 257, "M": 256}, {"B": 0}, {"M": 0}, {"E": 0}]),
    "edgl_adam_step": ("param grad m v n lr beta1 beta2 eps step_state l2 seg nseg shadow stream", ADAM_REQ, [L2_NO_SEG]),
    "edgl_step_begin": ("rng_state adam_state lr beta1 beta2 stream", ["rng_state", "adam_state"], []),
    "edgl_rng_advance": ("rng_state stream", ["rng_state"], []),
    "edgl_adam_apply": ("param grad m v n beta1 beta2 eps step_state l2 seg nseg shadow stream", ADAM_REQ, [L2_NO_SEG]),
    "edgl_adam_apply_l2p": ("param grad m v n beta1 beta2 eps step_state l2 seg nseg shadow l2_part stream", ADAM_REQ + ["l2_part"],
                            [L2_NO_SEG, {"nseg": 2}]),
    "edgl_adam_apply_ex": ("param grad m v n beta1 beta2 eps step_state l2 seg nseg shadow l2_part slabs_a stride_a lo_a hi_a zero_first_a "
                           "slabs_b stride_b lo_b hi_b nslab rng_cur step_next rng_next lr stream", ADAM_REQ,
                           [L2_NO_SEG,
                            # the next step's counters: all three pointers or none, in buffers of their own
                            {"rng_cur": ADDR}, {"step_next": ADDR2}, {"rng_next": ADDR2}, {"rng_cur": ADDR, "step_next": ADDR2},
                            {"step_next": ADDR2, "rng_next": ADDR2}, {"rng_cur": ADDR, "step_next": ADDR, "rng_next": ADDR2},
                            {"rng_cur": ADDR, "step_next": ADDR2, "rng_next": ADDR},
                            # slab ranges
                            {"nslab": -1}, {"nslab": 2}, {**SLAB_A, "nslab": -1}, {**SLAB_A, "lo_a": -4}, {**SLAB_A, "lo_a": 68},
                            {**SLAB_A, "hi_a": 4100}, {**SLAB_A, "stride_a": 60}, {**SLAB_B, "lo_b": -1}, {**SLAB_B, "lo_b": 65},
                            {**SLAB_B, "hi_b": 4100}, {**SLAB_B, "stride_b": 63}, {**SLAB_A, **SLAB_B, "hi_b": 4100}]),
    "edgl_l2_from_parts": ("l2_part nparts l2 out accumulate stream", ["l2_part", "out"], [{"nparts": 0}, {"nparts": -3}]),
    "edgl_l2_loss": ("param seg nseg l2 out accumulate workspace stream", ["param", "seg", "out", "workspace"], []),
    "edgl_reduce_partials": ("part P N ld out accumulate stream", ["part", "out"], [{"ld": 32}, {"P": 0}, {"N": 0}, {"N": 41}]),
    "edgl_reduce_ride": ("on", [], [{"on": 3}, {"on": -1}]),
}
# edgl_adam_apply_ex at THIS commit also refuses slabs with nslab = 0 (the parent launched: its vector path then read slab -1); the
# case is not in the parent's file, tests/test_cpu_misc_host.py holds it
NSLAB_ZERO = [{**SLAB_A, "nslab": 0}, {**SLAB_B, "nslab": 0}]


def call_args(name, override):
    arg_names, required, _ = SPECS[name]
    names = arg_names.split()
    good = {a: VALS[a] if a in VALS else (ADDR if a in required else None) for a in names}
    return tuple({**good, **override}[a] for a in names)


def rejection_cases():
    """[(entry point, case label, argument tuple)] in a fixed order"""
    out = []
    for name, (arg_names, required, own) in SPECS.items():
        cases = [("%s null" % a, {a: None}) for a in required]
        cases += [(" ".join("%s=%s" % kv for kv in ov.items()), ov) for ov in own]
        for label, ov in cases:
            out.append((name, label, call_args(name, ov)))
    return out


def call(lib, name, args):
    rc = getattr(lib, name)(*args)
    err = lib.edgl_last_error()
    return rc, err.decode() if err else None


def rejections(lib):
    """lib: easydgl_amd._lib.lib (argument types set from _lib.SIGNATURES)"""
    return [[name, label] + list(call(lib, name, args)) for name, label, args in rejection_cases()]


def queue(lib):
    return [lib.edgl_reduce_defer(1, None), lib.edgl_reduce_defer(-1, None)]


def main():
    sys.path.insert(0, ROOT)
    from easydgl_amd import _lib
    labels = [a for a in sys.argv[1:] if not a.startswith("--")]
    commit = labels[0] if labels else subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    rej = rejections(_lib.lib)
    passed = [r for r in rej if r[2] == 0]
    assert not passed, passed      # a recorded call must fail its validation
    out = {"commit": commit, "sizes": sizes(_lib.lib), "rejections": rej, "queue": queue(_lib.lib)}
    with open(PATH, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(PATH, len(rej), "rejections,", sum(len(v) for v in out["sizes"].values() if isinstance(v, dict)) + 1, "sizes at", commit)


if __name__ == "__main__":
    main()
