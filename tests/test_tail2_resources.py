"""The two-per-CU block-tail kernels (csrc/k_tail.hip, namespace t2) must fit their 128 registers WITHOUT scratch: a value reloaded
from scratch waits on vmcnt like any load, i.e. behind every output store issued before it — a full HBM write acknowledge per
store batch (the forward with 30 spilled registers ran 64.7 us at the headline shape, without them 49.5 us; DESIGN rule 80).
A spill is silent, so this test rebuilds the file's device code with the flags of build.py and reads the compiler's resource
remarks.  CPU only (hipcc cross-compiles)."""
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
    flags = b.FLAGS + b.EXTRA_FLAGS.get("k_tail.hip", [])
    r = subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                          os.path.join(ROOT, "easydgl_amd", "csrc", "k_tail.hip"), "-o", str(d / "k_tail.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return res


@pytest.mark.parametrize("kernel", ["tail2_fwd_kernelILi2E", "tail2_fwd_kernelILi4E", "tail2_fwd_kernelILi7E",
                                    "tail2_bwd_kernelILi2E", "tail2_bwd_kernelILi4E", "tail2_bwd_kernelILi7E"])
def test_two_per_cu_tail_kernels_have_no_scratch(tail_resources, kernel):
    hits = [v for k, v in tail_resources.items() if kernel in k]
    assert len(hits) == 1, (kernel, list(tail_resources))
    r = hits[0]
    print(kernel, r)
    assert r["VGPRs"] + r["AGPRs"] <= 128, r            # two workgroups of 512 threads per CU: four waves per SIMD
    assert r["Occupancy"] >= 4, r
    assert r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, r
