"""Outputs of the scoring / compaction / CE / tile-evaluation entry points (k_score.hip, k_ce.hip, k_eval_tile.hip) on fixed inputs,
for a bit-for-bit comparison of two builds of the library (the one to load is chosen by EDGL_LIB_PATH):

    EDGL_LIB_PATH=ab_libs/parent.so python tools/score_ab_dump.py OUT_A.npz
    python tools/score_ab_dump.py OUT_B.npz
    python tools/score_ab_dump.py --compare OUT_A.npz OUT_B.npz [--noise OUT_A2.npz]

Each dump runs in its own process.  --compare: every array must hold the same bits (floats are compared as integers, so NaN
payloads and signed zeros count); with --noise (a second dump of build A) an array that differs between A and A2 is reported as
run-to-run noise of the build itself, with its largest differences A / A2 and A / B, and does not fail the comparison.

Shapes: R = 300 rows of which 211 carry a label, I = 1037 items, item ranges [0, I) and [512, I); C / dtype = 32 f32, 32 bf16 (generic
kernels), 64 bf16 (one-launch row finish), 128 bf16 (strip), 256 bf16 (wide strip), 512 bf16 (wide finish).  The labels are DISTINCT,
so the f32-atomic one-hot scatter has one addend per table row and no summation order.  edgl_mask_topk: 4 rows of 1037 / 5000 /
10300 / 20480 logits (the three register forms and the LDS form), K = 10 and 128, tied values and a seen list; edgl_topk_merge:
S = 3, K = 100; edgl_rank_metrics: R = 70, K = 100."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

R, NW, I, I_MID = 300, 211, 1037, 512
CONFIGS = ((32, "f32"), (32, "bf16"), (64, "bf16"), (128, "bf16"), (256, "bf16"), (512, "bf16"))


def dump(path):
    import torch

    from easydgl_amd import ops
    from easydgl_amd._lib import check, lib

    p, st = ops._ptr, ops._stream()
    out = {}

    def keep(name, *tensors):
        torch.cuda.synchronize()
        for i, t in enumerate(tensors):
            a = t.detach().cpu()
            out["%s/%d" % (name, i)] = (a.view(torch.int16) if a.dtype == torch.bfloat16 else a).numpy().copy()

    def z(*shape, dtype=torch.float32):
        return torch.zeros(shape, device="cuda", dtype=dtype)

    g = np.random.default_rng(1234)
    labels_np = np.zeros(R, dtype=np.int64)
    labels_np[g.permutation(R)[:NW]] = g.permutation(np.arange(1, I))[:NW]
    labels = torch.tensor(labels_np).cuda()
    wtotal = torch.tensor([2 * NW + 3], dtype=torch.int32).cuda()
    gscale = torch.tensor([0.5], dtype=torch.float32).cuda()
    add1, add2 = torch.tensor([0.25]).cuda(), torch.tensor([0.125]).cuda()

    for C, dname in CONFIGS:
        dt = torch.float32 if dname == "f32" else torch.bfloat16
        tag = "C%d_%s" % (C, dname)
        rows = torch.tensor(g.standard_normal((R, C)) * 0.6, dtype=dt).cuda()
        tab = torch.tensor(g.standard_normal((I, C)) * 0.4, dtype=dt).cuda()
        bias = torch.tensor(g.standard_normal(I - 1) * 0.3, dtype=torch.float32).cuda()
        code = ops._code(rows)

        # ---- k_ce.hip: compaction ----
        perm, inv, nvalid = z(R, dtype=torch.int32), z(R, dtype=torch.int32), z(1, dtype=torch.int32)
        rows_c, lab_c = torch.zeros_like(rows), torch.zeros_like(labels)
        check(lib.edgl_compact_rows(p(rows), p(labels), R, C, p(perm), p(inv), p(nvalid), p(rows_c), p(lab_c), code, st), "compact_rows")
        keep(tag + "/compact_rows", perm, inv, nvalid, rows_c, lab_c)
        perm2, inv2, nv2, lab2 = z(R, dtype=torch.int32), z(R, dtype=torch.int32), z(1, dtype=torch.int32), torch.zeros_like(labels)
        check(lib.edgl_compact_scan(p(labels), R, p(perm2), p(inv2), p(nv2), st), "compact_scan")
        keep(tag + "/compact_scan", perm2, inv2, nv2)
        check(lib.edgl_compact_scan_labels(p(labels), R, p(perm2), p(inv2), p(nv2), p(lab2), st), "compact_scan_labels")
        keep(tag + "/compact_scan_labels", perm2, inv2, nv2, lab2)
        rows_g, lab_g = torch.zeros_like(rows), torch.zeros_like(labels)
        check(lib.edgl_compact_gather(p(rows), p(labels), p(perm2), R, C, p(rows_g), p(lab_g), code, st), "compact_gather")
        back = torch.zeros_like(rows)
        check(lib.edgl_scatter_rows(p(rows_g), p(inv2), R, C, p(back), code, st), "scatter_rows")
        keep(tag + "/gather_scatter", rows_g, lab_g, back)

        coef = None
        for i0, i1 in ((0, I), (I_MID, I)):
            rt = "%s/[%d,%d)" % (tag, i0, i1)
            n_it = i1 - i0
            # ---- two-pass kernels ----
            lse, ll, logits = z(R), z(R), z(R, n_it)
            ws = z(2 * R * lib.edgl_score_chunks(R, n_it))
            check(lib.edgl_score_lse_fwd(p(rows_c), p(tab), p(bias), p(lab_c), R, C, I, i0, i1, p(nvalid), p(lse), p(ll), p(logits), p(ws),
                                         code, st), "lse_fwd")
            keep(rt + "/lse_fwd", lse, ll, logits)
            if coef is None:      # the loss of the whole table; its lse and coefficients drive every backward below
                lse_all, loss, coef = lse, z(1), z(R)
                check(lib.edgl_ce_loss_fwd(p(lse), p(ll), p(lab_c), R, p(loss), p(coef), st), "ce_loss_fwd")
                loss2, coef2, loss3, coef3 = z(1), z(R), z(1), z(R)
                check(lib.edgl_ce_loss_fwd_add(p(lse), p(ll), p(lab_c), R, p(loss2), p(coef2), p(add1), p(add2), st), "ce_loss_fwd_add")
                check(lib.edgl_ce_loss_fwd_add_w(p(lse), p(ll), p(lab_c), R, p(loss3), p(coef3), p(add1), None, p(wtotal), st), "ce_loss_fwd_add_w")
                keep(tag + "/ce_loss", loss, coef, loss2, coef2, loss3, coef3)

            def grads():
                return torch.zeros_like(rows_c), z(I, C), z(I - 1)

            d_rows, d_tab, d_b = grads()
            ws = z(lib.edgl_score_bwd_workspace(R, C, I, n_it, code))
            check(lib.edgl_score_ce_bwd(p(rows_c), p(tab), p(bias), p(lab_c), p(lse_all), p(coef), None, R, C, I, i0, i1, p(nvalid), p(d_rows),
                                        p(d_tab), p(d_b), p(ws), code, st), "ce_bwd")
            keep(rt + "/ce_bwd", d_rows, d_tab, d_b)
            # ---- flash forward (three doors into the same pass) and the backward with d_rows ----
            nws = lib.edgl_score_flash_workspace(R, C, I, n_it, code)
            wsf = z(nws)
            lse1, ll1 = z(R), z(R)
            check(lib.edgl_score_flash_fwd(p(rows_c), p(tab), p(bias), p(lab_c), R, C, I, i0, i1, p(nvalid), p(lse1), p(ll1), p(wsf), code, st),
                  "flash_fwd")
            d_rows, d_tab, d_b = grads()
            check(lib.edgl_score_flash_bwd(p(rows_c), p(tab), p(bias), p(lab_c), p(lse_all), p(coef), p(gscale), R, C, I, i0, i1, p(nvalid),
                                           p(d_rows), p(d_tab), p(d_b), p(wsf), code, st), "flash_bwd")
            keep(rt + "/flash_fwd_bwd", lse1, ll1, d_rows, d_tab, d_b)
            for ready in (0, 1):
                wsp, lse2, ll2 = z(nws), z(R), z(R)
                if ready:
                    check(lib.edgl_score_prepare_table(p(tab), R, C, I, i0, i1, p(wsp), code, st), "prepare_table")
                check(lib.edgl_score_flash_fwd_pre(p(rows_c), p(tab), p(bias), p(lab_c), R, C, I, i0, i1, p(nvalid), p(lse2), p(ll2), p(wsp),
                                                   ready, code, st), "flash_fwd_pre")
                keep(rt + "/flash_fwd_pre%d" % ready, lse2, ll2)
            # ---- the table side alone, in its forms (the forward above left its slabs in wsf) ----
            for defer in (1, 3, 5):
                if defer == 5 and (i0, i1) != (0, I):
                    continue
                _, d_tab, d_b = grads()
                check(lib.edgl_score_flash_bwd_ex(p(rows_c), p(tab), p(bias), p(lab_c), p(lse_all), p(coef), None, R, C, I, i0, i1, p(nvalid),
                                                  None, p(d_tab), p(d_b), p(wsf), defer, code, st), "flash_bwd_ex")
                if defer == 5:
                    info = np.zeros(3, dtype=np.int64)
                    check(lib.edgl_score_flash_slab_info(R, C, I, n_it, code, info.ctypes.data), "slab_info")
                    o0, o1, ns = (int(v) for v in info)
                    keep(rt + "/flash_bwd_ex5", wsf[o0:o0 + ns * I * C], wsf[o1:o1 + ns * (I - 1)], d_tab, d_b)
                    continue
                keep(rt + "/flash_bwd_ex%d" % defer, d_tab, d_b)
                if defer == 1:
                    d_tab_det, d_b_det = d_tab.clone(), d_b.clone()
                    if dname == "bf16":
                        plan = ops.segsum_plan_buffer(R, I, "cuda")
                        check(lib.edgl_segsum_plan(p(lab_c), R, p(nvalid), I, i0, i1, p(plan), st), "segsum_plan")
                        check(lib.edgl_score_flash_label_term_det(p(rows_c), p(lab_c), p(coef), None, R, C, I, i0, i1, p(nvalid), p(d_tab_det),
                                                                  p(d_b_det), p(plan), code, st), "label_term_det")
                        keep(rt + "/label_term_det", d_tab_det, d_b_det)
                check(lib.edgl_score_flash_label_term(p(rows_c), p(lab_c), p(coef), None, R, C, I, i0, i1, p(nvalid), p(d_tab), p(d_b), code, st),
                      "label_term")
                keep(rt + "/label_term%d" % defer, d_tab, d_b)

        # ---- whole table, compacted rows: the forwards that write the coefficients / finish the rows ----
        nws = lib.edgl_score_flash_workspace(R, C, I, I, code)
        for name, wt in (("coef", None), ("coef_w", wtotal)):
            wsf, lse1, ll1, cf = z(nws), z(R), z(R), z(R)
            if wt is None:
                check(lib.edgl_score_flash_fwd_coef(p(rows_c), p(tab), p(bias), p(lab_c), R, C, I, p(nvalid), p(lse1), p(ll1), p(cf), p(wsf), code,
                                                    st), "fwd_coef")
            else:
                check(lib.edgl_score_flash_fwd_coef_w(p(rows_c), p(tab), p(bias), p(lab_c), R, C, I, p(nvalid), p(wt), p(lse1), p(ll1), p(cf),
                                                      p(wsf), code, st), "fwd_coef_w")
            d_rows, d_tab, d_b = (torch.zeros_like(rows_c), z(I, C), z(I - 1))
            check(lib.edgl_score_flash_bwd_ex(p(rows_c), p(tab), p(bias), p(lab_c), p(lse1), p(cf), None, R, C, I, 0, I, p(nvalid), p(d_rows),
                                              p(d_tab), p(d_b), p(wsf), 0, code, st), "flash_bwd_ex")
            keep("%s/fwd_%s" % (tag, name), lse1, ll1, cf, d_rows, d_tab, d_b)
        nparts = lib.edgl_score_ce_nparts(R, C)
        for name in ("rows_w", "rows_wp"):
            if name == "rows_wp" and nparts == 0:
                continue
            wsf, lse1, ll1, cf, d_rows = z(nws), z(R), z(R), z(R), torch.zeros_like(rows_c)
            part, loss = z(nparts + 1), z(1)
            if name == "rows_w":
                check(lib.edgl_score_flash_fwd_rows_w(p(rows_c), p(tab), p(bias), p(lab_c), R, C, I, p(nvalid), None, p(gscale), p(lse1), p(ll1),
                                                      p(cf), p(d_rows), p(wsf), code, st), "fwd_rows_w")
            else:
                check(lib.edgl_score_flash_fwd_rows_wp(p(rows_c), p(tab), p(bias), p(lab_c), R, C, I, p(nvalid), p(wtotal), None, p(lse1), p(ll1),
                                                       p(cf), p(d_rows), p(part), p(wsf), code, st), "fwd_rows_wp")
                check(lib.edgl_ce_loss_parts(p(part), nparts, p(loss), p(add1), p(add2), p(wtotal), st), "ce_loss_parts")
            d_tab, d_b = z(I, C), z(I - 1)
            check(lib.edgl_score_flash_bwd(p(rows_c), p(tab), p(bias), p(lab_c), p(lse1), p(cf), p(gscale) if name == "rows_w" else None, R, C, I,
                                           0, I, p(nvalid), None, p(d_tab), p(d_b), p(wsf), code, st), "flash_bwd")
            keep("%s/fwd_%s" % (tag, name), lse1, ll1, cf, d_rows, part, loss, d_tab, d_b)

    # ---- k_eval_tile.hip ----
    i0 = 8
    for n in (1037, 5000, 10300, 20480):
        logits = torch.tensor(np.round(g.standard_normal((4, n)) * 4) / 4, dtype=torch.float32).cuda()      # many tied values
        seen_np = g.integers(i0 - 4, i0 + n + 4, size=(4, 50))
        seen_np[:, :3] = 0
        seen = torch.tensor(seen_np, dtype=torch.int64).cuda()
        for K in (10, 128):
            for sname, s in (("seen", seen), ("all", None)):
                x = logits.clone()
                val, idx = ops.mask_topk(x, i0, s, K)
                keep("mask_topk/n%d_K%d_%s" % (n, K, sname), val, idx, x)
    S, Rm, K = 3, 70, 100
    cval = torch.tensor(np.round(g.standard_normal((S, Rm, K)) * 4) / 4, dtype=torch.float32).cuda()
    cidx_np = g.integers(0, 400, size=(S, Rm, K)).astype(np.int32)
    cidx_np[g.random((S, Rm, K)) < 0.05] = -1
    cval_np = cval.cpu().numpy()
    cval_np[cidx_np < 0] = -np.inf
    val, idx = ops.topk_merge(torch.tensor(cval_np).cuda(), torch.tensor(cidx_np).cuda())
    keep("topk_merge", val, idx)
    label = torch.tensor(g.integers(0, 400, size=Rm), dtype=torch.int64).cuda()
    metrics = z(6)
    ops.rank_metrics(idx.contiguous(), label, metrics)
    ops.rank_metrics(idx.contiguous(), idx[:, 7].to(torch.int64).contiguous(), metrics)      # (labels that are in the lists)
    keep("rank_metrics", metrics)

    np.savez(path, **out)
    print("wrote", path, len(out), "arrays")


def bits(a):
    return a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def maxdiff(a, b):
    with np.errstate(invalid="ignore"):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    return float(np.nanmax(d)) if d.size else 0.0


def compare(path_a, path_b, path_noise):
    A, B = np.load(path_a), np.load(path_b)
    N = np.load(path_noise) if path_noise else None
    assert set(A.files) == set(B.files), set(A.files) ^ set(B.files)
    same, noisy, bad = 0, [], []
    for k in sorted(A.files):
        if A[k].shape == B[k].shape and np.array_equal(bits(A[k]), bits(B[k])):
            same += 1
        elif N is not None and not np.array_equal(bits(A[k]), bits(N[k])):
            noisy.append((k, maxdiff(A[k], N[k]), maxdiff(A[k], B[k]), float(np.abs(A[k]).max())))
        else:
            bad.append((k, maxdiff(A[k], B[k])))
    if N is not None:      # (an array may be noisy and still happen to agree between A and B)
        also = [k for k in sorted(A.files) if not np.array_equal(bits(A[k]), bits(N[k])) and k not in [n[0] for n in noisy]]
        print("differ between the two dumps of build A but not between A and B:", also)
    print("%d arrays, %d identical, %d run-to-run noise, %d DIFFERENT" % (len(A.files), same, len(noisy), len(bad)))
    for k, dn, db, mx in noisy:
        print("  noise      %-50s max |A - A2| %.3e   max |A - B| %.3e   max |A| %.3e" % (k, dn, db, mx))
    for k, d in bad:
        print("  DIFFERENT  %-50s max |A - B| %.3e" % (k, d))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--compare":
        compare(args[1], args[2], args[4] if len(args) > 4 and args[3] == "--noise" else None)
    elif len(args) == 1:
        dump(args[0])
    else:
        sys.exit(__doc__)
