"""Generates tests/golden/score_host_parent.json — what the HOST side of the scoring / compaction / CE / top-K entry points answers.

Two kinds of records, none of which reaches a kernel launch (so they need no GPU):
  plans        edgl_score_chunks, edgl_score_bwd_workspace, edgl_score_flash_workspace, the three values of
               edgl_score_flash_slab_info and edgl_score_ce_nparts over a grid of shapes — engines cache these numbers.  Taken in
               fresh child processes, once with the default switches and once with the strip kernels switched off
               (EDGL_SCORE_STRIP / STRIPW / STRIPW512 = 0: the switches are latched per process).
  rejections   (return code, edgl_last_error text) of calls that fail argument validation: all pointers null, each required
               pointer null in turn, a bad dtype / width / range / row count, and the special cases of single entry points.
               Pointers that must be non-null are the dummy address ADDR: every call listed here fails before it is used.
               Only add a case after reading the entry point's checks — a call that passes them would launch on that address.

The file records what the library did at the commit named in it; tests/test_cpu_score_host.py replays the same calls against
the built library and compares exactly.  Regenerate only on purpose, with the library of a clean checkout:

    python tests/golden/make_score_host.py [commit label]
"""
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "score_host_parent.json")

RS = (1, 7, 255, 256, 257, 5370, 10240, 20480)
CS = (32, 64, 128, 256, 512)
IS = (2, 41, 20001, 1000001)
STRIP_OFF = {"EDGL_SCORE_STRIP": "0", "EDGL_SCORE_STRIPW": "0", "EDGL_SCORE_STRIPW512": "0"}
MODES = {"default": {}, "strips_off": STRIP_OFF}


def item_counts(I):
    """the whole table, and a shard of about I / 8 items rounded up to 8 (I = 2: the empty shard)"""
    return sorted({I, min(I, (I // 8 + 7) // 8 * 8)})


def load_plain():
    """the library without torch, for the plan queries of a child process (integers in, integers out)"""
    lib = ctypes.CDLL(os.environ.get("EDGL_LIB_PATH") or os.path.join(ROOT, "easydgl_amd", "libeasydgl_hip.so"))
    lib.edgl_score_bwd_workspace.restype = ctypes.c_long
    lib.edgl_score_flash_workspace.restype = ctypes.c_long
    lib.edgl_score_flash_slab_info.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p]
    return lib


def plans(lib):
    out = {"chunks": {}, "nparts": {}, "plan": {}}
    slab = (ctypes.c_long * 3)()
    for R in RS:
        for C in CS:
            out["nparts"]["%d,%d" % (R, C)] = lib.edgl_score_ce_nparts(R, C)
        for I in IS:
            for n in item_counts(I):
                out["chunks"]["%d,%d" % (R, n)] = lib.edgl_score_chunks(R, n)
                for C in CS:
                    for dtype in (0, 1):
                        rc = lib.edgl_score_flash_slab_info(R, C, I, n, dtype, ctypes.addressof(slab))
                        out["plan"]["%d,%d,%d,%d,%d" % (R, C, I, n, dtype)] = [
                            lib.edgl_score_bwd_workspace(R, C, I, n, dtype), lib.edgl_score_flash_workspace(R, C, I, n, dtype),
                            rc, slab[0], slab[1], slab[2]]
    return out


def plans_in_child(mode):
    env = {k: v for k, v in os.environ.items() if k not in STRIP_OFF}
    env.update(MODES[mode])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plans"], env=env, capture_output=True, text=True, check=True)
    return json.loads(r.stdout)


# ---- rejections ---------------------------------------------------------------------------------------------------------------
ADDR = 4096      # non-null and 16-byte aligned (check_score tests the alignment before the width)
INTS = {"R": 24, "C": 32, "I": 41, "i0": 0, "i1": 41, "dtype": 0, "table_ready": 0, "defer": 0, "n": 41, "T": 0, "K": 10, "S": 3,
        "nparts": 4, "n_items": 41}
SCORE = ["rows", "table", "out_bias"]
# name: (arguments in ABI order, pointers that must be non-null, generic bad values that the entry point checks, own cases)
SPECS = {
    "edgl_score_lse_fwd": ("rows table out_bias labels R C I i0 i1 nvalid row_lse label_logit logits workspace dtype stream",
                           SCORE + ["labels", "row_lse", "label_logit", "workspace"], "dtype C i0 i1 R", []),
    "edgl_score_ce_bwd": ("rows table out_bias labels row_lse coef gscale R C I i0 i1 nvalid d_rows d_table d_bias workspace dtype stream",
                          SCORE + ["labels", "row_lse", "coef", "d_rows", "d_table", "d_bias", "workspace"], "dtype C i0 i1 R", []),
    "edgl_score_flash_fwd": ("rows table out_bias labels R C I i0 i1 nvalid row_lse label_logit workspace dtype stream",
                             SCORE + ["labels", "row_lse", "label_logit", "workspace"], "dtype C i0 i1 R", []),
    "edgl_score_flash_fwd_pre": ("rows table out_bias labels R C I i0 i1 nvalid row_lse label_logit workspace table_ready dtype stream",
                                 SCORE + ["labels", "row_lse", "label_logit", "workspace"], "dtype C i0 i1 R", [{"table_ready": 1, "labels": None}]),
    "edgl_score_flash_fwd_coef": ("rows table out_bias labels R C I nvalid row_lse label_logit coef workspace dtype stream",
                                  SCORE + ["labels", "nvalid", "row_lse", "label_logit", "coef", "workspace"], "dtype C R", []),
    "edgl_score_flash_fwd_coef_w": ("rows table out_bias labels R C I nvalid wtotal row_lse label_logit coef workspace dtype stream",
                                    SCORE + ["labels", "nvalid", "row_lse", "label_logit", "coef", "workspace"], "dtype C R", []),
    "edgl_score_flash_fwd_rows_w": ("rows table out_bias labels R C I nvalid wtotal gscale row_lse label_logit coef d_rows workspace dtype stream",
                                    SCORE + ["labels", "nvalid", "row_lse", "label_logit", "coef", "d_rows", "workspace"], "dtype C R", []),
    "edgl_score_flash_fwd_rows_wp": ("rows table out_bias labels R C I nvalid wtotal gscale row_lse label_logit coef d_rows ce_part workspace dtype stream",
                                     SCORE + ["labels", "nvalid", "row_lse", "label_logit", "coef", "d_rows", "workspace"], "dtype C R",
                                     [{"ce_part": ADDR}, {"ce_part": ADDR, "d_rows": None}, {"ce_part": ADDR, "C": 48}]),   # C = 32 has no loss parts
    "edgl_score_flash_bwd": ("rows table out_bias labels row_lse coef gscale R C I i0 i1 nvalid d_rows d_table d_bias workspace dtype stream",
                             SCORE + ["labels", "row_lse", "coef", "d_table", "d_bias", "workspace"], "dtype C i0 i1 R", []),
    "edgl_score_flash_bwd_ex": ("rows table out_bias labels row_lse coef gscale R C I i0 i1 nvalid d_rows d_table d_bias workspace defer dtype stream",
                                SCORE + ["labels", "row_lse", "coef", "d_table", "d_bias", "workspace"], "dtype C i0 i1 R",
                                [{"defer": 7, "workspace": None}]),
    "edgl_score_prepare_table": ("table R C I i0 i1 workspace dtype stream", ["table", "workspace"], "dtype", []),
    "edgl_score_flash_label_term": ("rows labels coef gscale R C I i0 i1 nvalid d_table d_bias dtype stream",
                                    ["rows", "labels", "coef", "d_table", "d_bias"], "i1 R", []),
    "edgl_score_flash_label_term_det": ("rows labels coef gscale R C I i0 i1 nvalid d_table d_bias plan dtype stream",
                                        ["rows", "labels", "coef", "d_table", "d_bias", "plan"], "dtype i1 R", []),
    "edgl_score_flash_slab_info": ("R C I n_items dtype out", ["out"], "dtype", []),
    "edgl_compact_scan": ("labels R perm inv nvalid stream", ["labels", "perm", "inv", "nvalid"], "R", []),
    "edgl_compact_scan_labels": ("labels R perm inv nvalid labels_c stream", ["labels", "perm", "inv", "nvalid", "labels_c"], "R", []),
    "edgl_compact_gather": ("rows labels perm R C rows_c labels_c dtype stream", ["rows", "labels", "perm", "rows_c", "labels_c"], "dtype R",
                            [{"C": 33}, {"C": 36, "dtype": 1}]),
    # (a bad dtype or width passes edgl_compact_rows' own checks and is found behind the scan's launch: not recorded)
    "edgl_compact_rows": ("rows labels R C perm inv nvalid rows_c labels_c dtype stream",
                          ["rows", "labels", "perm", "inv", "nvalid", "rows_c", "labels_c"], "R", []),
    "edgl_scatter_rows": ("rows_c inv R C rows dtype stream", ["rows_c", "inv", "rows"], "dtype", []),
    "edgl_ce_loss_fwd": ("row_lse label_logit labels R loss_out coef stream", ["row_lse", "label_logit", "labels", "loss_out"], "", []),
    "edgl_ce_loss_fwd_add": ("row_lse label_logit labels R loss_out coef add_in add_in2 stream",
                             ["row_lse", "label_logit", "labels", "loss_out"], "", []),
    "edgl_ce_loss_fwd_add_w": ("row_lse label_logit labels R loss_out coef add_in add_in2 wtotal stream",
                               ["row_lse", "label_logit", "labels", "loss_out"], "", []),
    "edgl_ce_loss_parts": ("ce_part nparts loss_out add_in add_in2 wtotal stream", ["ce_part", "loss_out"], "", [{"nparts": 0}]),
    "edgl_mask_topk": ("logits R n i0 seen T K out_val out_idx stream", ["logits", "out_val", "out_idx"], "R", [{"K": 200}, {"K": 0}, {"n": 0}]),
    "edgl_topk_merge": ("cand_val cand_idx S R K out_val out_idx stream", ["cand_val", "cand_idx", "out_val", "out_idx"], "R",
                        [{"S": 11, "K": 100}, {"S": 0}]),
    "edgl_rank_metrics": ("topk_idx R K label metrics stream", ["topk_idx", "label", "metrics"], "", []),
}
GENERIC = {"dtype": {"dtype": 7}, "C": {"C": 48}, "i0": {"i0": 4}, "i1": {"i1": 42}, "R": {"R": 0}}


def rejection_cases():
    """[(entry point, case label, argument tuple)] in a fixed order"""
    out = []
    for name, (arg_names, required, generic, own) in SPECS.items():
        names = arg_names.split()
        good = {a: INTS[a] if a in INTS else (ADDR if a in required else None) for a in names}
        cases = [("all null", {a: None for a in names if a not in INTS})]
        cases += [("%s null" % a, {a: None}) for a in required]
        if name == "edgl_score_lse_fwd":      # labels are optional there (they only make label_logit required): a VALID call
            cases = [c for c in cases if c[0] != "labels null"]
        cases += [(" ".join("%s=%s" % kv for kv in ov.items()), ov) for ov in [GENERIC[g] for g in generic.split()] + own]
        for label, ov in cases:
            out.append((name, label, tuple({**good, **ov}[a] for a in names)))
    return out


def rejections(lib):
    """lib: easydgl_amd._lib.lib (argument types set from _lib.SIGNATURES)"""
    out = []
    for name, label, args in rejection_cases():
        rc = getattr(lib, name)(*args)
        err = lib.edgl_last_error()
        out.append([name, label, rc, err.decode() if err else None])
    return out


def main():
    if "--plans" in sys.argv:
        json.dump(plans(load_plain()), sys.stdout)
        return
    sys.path.insert(0, ROOT)
    from easydgl_amd import _lib
    labels = [a for a in sys.argv[1:] if not a.startswith("--")]
    commit = labels[0] if labels else subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    rej = rejections(_lib.lib)
    passed = [r for r in rej if r[2] == 0]
    assert not passed, passed      # a recorded call must fail its validation
    out = {"commit": commit, "plans": {m: plans_in_child(m) for m in MODES}, "rejections": rej}
    with open(PATH, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(PATH, len(rej), "rejections,", sum(len(p["plan"]) for p in out["plans"].values()), "plans at", commit)


if __name__ == "__main__":
    main()
