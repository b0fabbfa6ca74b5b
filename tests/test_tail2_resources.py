"""The two-per-CU block-tail kernels (csrc/k_tail_fwd.hip and k_tail_bwd.hip, namespace t2) must fit their 128 registers WITHOUT
scratch: a value reloaded from scratch waits on vmcnt like any load, i.e. behind every output store issued before it — a full HBM
write acknowledge per store batch (the forward with 30 spilled registers ran 64.7 us at the headline shape, without them 49.5 us;
DESIGN rule 80).  The one-per-CU kernels of the same units own their 256 registers, and must not spill either ("256, no spills" in
DESIGN's kernel table).  A spill is silent, so this test rebuilds the two units' device code with the flags of build.py and reads
the compiler's resource remarks: the forward kernels' from one unit, the backward kernels' from the other.  CPU only (hipcc
cross-compiles)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def tail_resources(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    import importlib.util
    spec = importlib.util.spec_from_file_location("_edgl_build_tail", os.path.join(ROOT, "easydgl_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    d = tmp_path_factory.mktemp("tail_res")
    procs = []
    for unit in ("k_tail_fwd", "k_tail_bwd"):      # both compiles at once
        flags = b.FLAGS + b.EXTRA_FLAGS.get(unit + ".hip", [])
        procs.append(subprocess.Popen([HIPCC] + flags + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                                        os.path.join(ROOT, "easydgl_amd", "csrc", unit + ".hip"), "-o", str(d / (unit + ".o"))],
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    remarks = []
    for pr in procs:
        err = pr.communicate()[1]
        assert pr.returncode == 0, err[-3000:]
        remarks += err.splitlines()
    res, cur = {}, None
    for line in remarks:
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return res


TWO_PER_CU = ["tail2_fwd_kernelILi2E", "tail2_fwd_kernelILi4E", "tail2_fwd_kernelILi7E",
              "tail2_bwd_kernelILi2E", "tail2_bwd_kernelILi4E", "tail2_bwd_kernelILi7E"]
ONE_PER_CU = ["tail_%s_kernelILi%dELi%dE" % (d, ct, nrt) for d in ("fwd", "bwd") for ct in (4, 8) for nrt in (2, 4, 7)]


@pytest.mark.parametrize("kernel", TWO_PER_CU + ONE_PER_CU)
def test_two_per_cu_tail_kernels_have_no_scratch(tail_resources, kernel):
    hits = [v for k, v in tail_resources.items() if kernel in k]
    assert len(hits) == 1, (kernel, list(tail_resources))
    r = hits[0]
    print(kernel, r)
    if kernel in TWO_PER_CU:
        assert r["VGPRs"] + r["AGPRs"] <= 128, r            # two workgroups of 512 threads per CU: four waves per SIMD
        assert r["Occupancy"] >= 4, r
    assert r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, r
