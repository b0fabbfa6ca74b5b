"""Outputs of the TPP / optimizer / reduction entry points (k_tpp.hip, k_optim.hip, k_reduce.hip) on fixed inputs, for a bit-for-bit
comparison of two builds of the library (the one to load is chosen by EDGL_LIB_PATH):

    EDGL_LIB_PATH=ab_libs/parent.so python tools/misc_ab_dump.py OUT_A.npz
    python tools/misc_ab_dump.py OUT_B.npz
    python tools/misc_ab_dump.py --compare OUT_A.npz OUT_B.npz [--noise OUT_A2.npz]

Each dump runs in its own process.  --compare: every array must hold the same bits (floats are compared as integers, so NaN
payloads and signed zeros count); with --noise (a second dump of build A) an array that differs between A and A2 is reported as
run-to-run noise of the build itself, with its largest differences A / A2 and A / B, and does not fail the comparison.

Shapes: B = 6, T = 21, H = 3, NI = 40 items.  TPP: E in {5, 16, 20} marks, M in {4, 20} masked slots with one position drawn twice,
and the all-position mode (M = T); the one-launch per-sequence form and the slot data exist for E <= 16 / E = 16 only.  edgl_tpp_norm
also at B = 258, M = 255 (65 790 labels: the multi-workgroup form).  Adam: n = 4099 elements, three steps, with and without the bf16
shadow, 2 and 5 l2 segments; edgl_adam_apply_ex with a 4-aligned slab range (3 slabs, zero_first = 4), a range of odd stride and the
next step's counters.  Reductions: P in {7, 40, 1616} partial rows, N in {33, 1024} columns, overwrite and accumulate, and a
deferred list flushed in the vector form and in both scalar forms."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, T, H, NI = 6, 21, 3, 40
N_ADAM = 4099


def dump(path):
    import torch

    from easydgl_amd import ops
    from easydgl_amd._lib import check, lib
    from oracle import easydgl_oracle as O

    p, st = ops._ptr, ops._stream()
    out = {}

    def keep(name, *tensors):
        torch.cuda.synchronize()
        for i, t in enumerate(tensors):
            a = t.detach().cpu()
            out["%s/%d" % (name, i)] = (a.view(torch.int16) if a.dtype == torch.bfloat16 else a).numpy().copy()

    def z(*shape, dtype=torch.float32):
        return torch.zeros(shape, device="cuda", dtype=dtype)

    def dev(a, dtype=None):
        return torch.tensor(np.asarray(a), dtype=dtype).cuda()

    g = np.random.default_rng(4321)
    coef = 0.41
    gscale = dev([0.5], torch.float32)

    # ---- k_tpp.hip ----
    for E in (5, 16, 20):
        mt = dev(O.synthetic_mark_table(NI, E, multi_hot=True).astype(np.uint8))
        for M, masked in ((4, True), (20, True), (T, False)):
            tag = "tpp/E%d_M%d_%s" % (E, M, "masked" if masked else "allpos")
            lam = dev(g.uniform(0.2, 2.0, size=(H * B, T, E)), torch.float32)
            labels_np = g.integers(1, NI, size=(B, M))
            labels_np[0, 0] = 0
            mp = None
            if masked:
                mpn = np.stack([g.choice(T - 1, M, replace=False) + 1 for _ in range(B)])
                mpn[1, 2] = mpn[1, 0]                         # the same position twice, two different labels
                mpn[2, 3] = mpn[2, 1]; labels_np[2, 3] = 0    # ... and once as a zero-weight padding slot
                mp = dev(mpn, torch.int64)
            labels = dev(labels_np, torch.int64)
            ts = dev(np.cumsum(g.exponential(40.0, size=(B, T if masked else T + 1)), axis=1) + 9.5e8, torch.float32)
            nws = int(max(lib.edgl_tpp_workspace(), lib.edgl_tpp_rows_workspace(B, H, M)))

            sums, reg, dlam = z(nws), torch.full((1,), 3.0, device="cuda"), z(H * B, T, E)
            check(lib.edgl_tpp_fwd(p(lam), p(mp), p(labels), p(ts), p(mt), B, T, H, E, M, coef, p(sums), p(reg), 1, st), "tpp_fwd")
            check(lib.edgl_tpp_bwd(p(lam), p(mp), p(labels), p(ts), p(mt), B, T, H, E, M, coef, p(sums), p(gscale), p(dlam), st), "tpp_bwd")
            keep(tag + "/fwd_bwd_pair", sums[:4], reg, dlam)
            if E <= 16:
                sums, reg, dlam = z(nws), z(1), torch.full((H * B, T, E), float("nan"), device="cuda")
                check(lib.edgl_tpp_fwd_bwd(p(lam), p(mp), p(labels), p(ts), p(mt), B, T, H, E, M, coef, p(sums), p(reg), 0, p(dlam), st),
                      "tpp_fwd_bwd")
                keep(tag + "/fwd_bwd", sums[:8], reg, dlam)
            sums, reg, dlam = z(nws), z(1), z(H * B, T, E)
            check(lib.edgl_tpp_norm(p(labels), p(mt), B, M, E, p(sums), st), "tpp_norm")
            keep(tag + "/norm", sums[:8].view(torch.int32))
            check(lib.edgl_tpp_fwd_bwd_rows(p(lam), p(mp), p(labels), p(ts), p(mt), B, T, H, E, M, coef, p(sums), p(reg), 0, p(dlam), st),
                  "tpp_fwd_bwd_rows")
            keep(tag + "/rows", sums[:8], reg, dlam)
            counts = z(2, dtype=torch.int32)
            check(lib.edgl_dp_counts(p(labels), p(mt), B, M, E, p(counts), st), "dp_counts")
            keep(tag + "/dp_counts", counts)
            if E == 16 and masked:
                desc = z(int(lib.edgl_tpp_prep_bytes(B, T, M)), dtype=torch.uint8)
                check(lib.edgl_tpp_prep(p(mp), p(labels), p(ts), p(mt), B, T, E, M, p(desc), st), "tpp_prep")
                keep(tag + "/prep", desc)
                for nparts in (H * B, 9000):
                    part = dev(g.standard_normal((nparts + 1, 2)), torch.float32)
                    part[nparts].view(torch.int32)[0] = 1234 + nparts      # the normaliser edgl_tpp_finish_parts_n reads
                    for acc in (0, 1):
                        sums, reg = z(nws), torch.full((1,), 3.0, device="cuda")
                        check(lib.edgl_tpp_finish_parts(p(part), nparts, coef, H, p(desc), B, T, M, p(sums), p(reg), acc, st), "finish_parts")
                        keep(tag + "/finish_parts_desc_n%d_a%d" % (nparts, acc), sums[:8], reg)
                        sums.view(torch.int32)[4] = 777
                        check(lib.edgl_tpp_finish_parts(p(part), nparts, coef, H, None, B, T, M, p(sums), p(reg), acc, st), "finish_parts")
                        keep(tag + "/finish_parts_sums_n%d_a%d" % (nparts, acc), sums[:8], reg)
                        check(lib.edgl_tpp_finish_parts_n(p(part), nparts, coef, H, p(sums), p(reg), acc, st), "finish_parts_n")
                        keep(tag + "/finish_parts_n_n%d_a%d" % (nparts, acc), sums[:8], reg)
    for E in (16, 5):      # 65 790 labels: the multi-workgroup count
        Bn, Mn = 258, 255
        mt = dev(O.synthetic_mark_table(NI, E, multi_hot=True).astype(np.uint8))
        labels = dev(g.integers(0, NI, size=(Bn, Mn)), torch.int64)
        sums = z(8)
        for rep in range(2):
            check(lib.edgl_tpp_norm(p(labels), p(mt), Bn, Mn, E, p(sums), st), "tpp_norm")
            keep("tpp/norm_big_E%d_%d" % (E, rep), sums.view(torch.int32))

    # ---- k_optim.hip ----
    n = N_ADAM
    w0, g0 = g.standard_normal(n), g.standard_normal(n) * 0.1
    nl2 = int(lib.edgl_adam_l2_parts(n))
    segs = {2: [[0, 1000], [2048, 3000]], 5: [[0, 500], [600, 601], [1000, 2047], [2050, 3000], [4000, 4099]]}
    lr, b1, b2, eps, l2 = 1e-2, 0.9, 0.999, 1e-8, 0.01
    for entry in ("step", "apply", "apply_l2p", "apply_ex", "apply_ex_plain"):
        for use_shadow in (True, False):
            for nseg in (2, 5):
                tag = "adam/%s_sh%d_seg%d" % (entry, use_shadow, nseg)
                w, m, v = dev(w0, torch.float32), z(n), z(n)
                shadow = z(n, dtype=torch.bfloat16) if use_shadow else None
                seg = dev(segs[nseg], torch.int64)
                state = [z(2, dtype=torch.int64), z(2, dtype=torch.int64)]      # Adam step + learning rate: current, next
                rng = [dev([1234, 7], torch.int64), z(2, dtype=torch.int64)]
                l2p = torch.full((nl2,), float("nan"), device="cuda")
                slab_a, slab_b = dev(g.standard_normal(3 * 512), torch.float32), dev(g.standard_normal(3 * 77), torch.float32)
                if entry.startswith("apply_ex"):
                    check(lib.edgl_step_begin(p(rng[0]), p(state[0]), lr, b1, b2, st), "step_begin")
                for t in range(1, 4):
                    gt = dev(g0 * t, torch.float32)
                    if entry == "step":
                        check(lib.edgl_adam_step(p(w), p(gt), p(m), p(v), n, lr, b1, b2, eps, p(state[0]), l2, p(seg), nseg, p(shadow), st),
                              "adam_step")
                    elif entry in ("apply", "apply_l2p"):
                        check(lib.edgl_step_begin(p(rng[0]), p(state[0]), lr, b1, b2, st), "step_begin")
                        if entry == "apply":
                            check(lib.edgl_adam_apply(p(w), p(gt), p(m), p(v), n, b1, b2, eps, p(state[0]), l2, p(seg), nseg, p(shadow), st),
                                  "adam_apply")
                        else:
                            check(lib.edgl_adam_apply_l2p(p(w), p(gt), p(m), p(v), n, b1, b2, eps, p(state[0]), l2, p(seg), nseg, p(shadow),
                                                          p(l2p), st), "adam_apply_l2p")
                    elif entry == "apply_ex":
                        check(lib.edgl_adam_apply_ex(p(w), p(gt), p(m), p(v), n, b1, b2, eps, p(state[0]), l2, p(seg), nseg, p(shadow), p(l2p),
                                                     p(slab_a), 512, 1024, 1536, 4, p(slab_b), 77, 3001, 3078, 3,
                                                     p(rng[0]), p(state[1]), p(rng[1]), lr, st), "adam_apply_ex")
                        keep(tag + "/grad_t%d" % t, gt)
                        state.reverse(); rng.reverse()
                    else:
                        check(lib.edgl_adam_apply_ex(p(w), p(gt), p(m), p(v), n, b1, b2, eps, p(state[0]), l2, p(seg), nseg, p(shadow), None,
                                                     None, 0, 0, 0, 0, None, 0, 0, 0, 0, None, None, None, lr, st), "adam_apply_ex")
                        check(lib.edgl_step_begin(p(rng[0]), p(state[0]), lr, b1, b2, st), "step_begin")
                    keep(tag + "/t%d" % t, w, m, v, state[0], state[1], rng[0], rng[1], l2p, *([shadow] if use_shadow else []))
                if entry == "apply_l2p" and use_shadow:
                    for acc in (0, 1):
                        o1, o2, ws = torch.full((1,), 3.0, device="cuda"), torch.full((1,), 3.0, device="cuda"), z(1024)
                        check(lib.edgl_l2_from_parts(p(l2p), nl2, l2, p(o1), acc, st), "l2_from_parts")
                        check(lib.edgl_l2_loss(p(w), p(seg), nseg, l2, p(o2), acc, p(ws), st), "l2_loss")
                        keep("l2/seg%d_a%d" % (nseg, acc), o1, o2, ws)
    rng_s, adam_s = dev([99, 5], torch.int64), z(2, dtype=torch.int64)
    for t in range(3):
        check(lib.edgl_step_begin(p(rng_s), p(adam_s), 3e-3, b1, b2, st), "step_begin")
        keep("step_begin/%d" % t, rng_s, adam_s)
    check(lib.edgl_rng_advance(p(rng_s), st), "rng_advance")
    keep("rng_advance", rng_s)

    # ---- k_reduce.hip ----
    for P in (7, 40, 1616):
        for N in (33, 1024):
            ld = N + 3 if N == 33 else N
            part = dev(g.standard_normal((P, ld)), torch.float32)
            for acc in (0, 1):
                o = torch.full((N,), 0.25, device="cuda")
                check(lib.edgl_reduce_partials(p(part), P, N, ld, p(o), acc, st), "reduce_partials")
                keep("reduce/P%d_N%d_a%d" % (P, N, acc), o)
    lists = {"vec": ((7, 1024, 1024), (40, 64, 64), (1616, 32, 36)),           # every job in the float4 form
             "scalar8": ((7, 1024, 1024), (40, 33, 36), (600, 64, 64)),        # one job outside it, no deep job
             "scalar32": ((7, 1024, 1024), (40, 33, 36), (1616, 32, 32))}      # ... and a deep job: 32 row lanes
    for name, jobs in lists.items():
        parts = [dev(g.standard_normal((P, ld)), torch.float32) for P, N, ld in jobs]
        outs = [torch.full((N,), 0.25, device="cuda") for P, N, ld in jobs]
        check(lib.edgl_reduce_defer(1, st), "reduce_defer")
        try:
            for (P, N, ld), part, o in zip(jobs, parts, outs):
                check(lib.edgl_reduce_partials(p(part), P, N, ld, p(o), 0, st), "reduce_partials")
            check(lib.edgl_reduce_flush(st), "reduce_flush")
            check(lib.edgl_reduce_defer(0, st), "reduce_defer")
        except Exception:
            lib.edgl_reduce_defer(-1, st)
            raise
        keep("reduce/deferred_" + name, *outs)

    np.savez(path, **out)
    print("wrote", path, len(out), "arrays")


def bits(a):
    return a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def maxdiff(a, b):
    with np.errstate(invalid="ignore"):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    return float(np.nanmax(d)) if d.size else 0.0


def compare(path_a, path_b, path_noise):
    A, Bf = np.load(path_a), np.load(path_b)
    N = np.load(path_noise) if path_noise else None
    assert set(A.files) == set(Bf.files), set(A.files) ^ set(Bf.files)
    same, noisy, bad = 0, [], []
    for k in sorted(A.files):
        if A[k].shape == Bf[k].shape and np.array_equal(bits(A[k]), bits(Bf[k])):
            same += 1
        elif N is not None and not np.array_equal(bits(A[k]), bits(N[k])):
            noisy.append((k, maxdiff(A[k], N[k]), maxdiff(A[k], Bf[k]), float(np.abs(A[k]).max())))
        else:
            bad.append((k, maxdiff(A[k], Bf[k])))
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
