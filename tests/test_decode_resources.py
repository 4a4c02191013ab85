"""Register budget of the decode-attention kernels, from the compiler's
resource-usage remarks (hipcc cross-compiles gfx950 without a GPU, so this
runs in CPU CI). attn_decode.hip's kernels are compositions of shared
force-inlined stages, and the register allocator is sensitive to how those
are written: a change that spills, or that drops the fused kernel under the
4 waves/SIMD it is built for, shows here before it reaches a GPU."""
import os
import re
import shutil
import subprocess

import pytest

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC_ATTN = os.path.join(REPO, "bee2bee_amd", "ops", "csrc", "attn_decode.hip")

# G in 1..8 and 16: generic scores 36, MFMA scores 108, PV 72, combine 18,
# fused 216
N_KERNELS = 450


def resource_remarks(stderr):
    """{kernel symbol: {field: value}} from -Rpass-analysis remarks."""
    out, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z /]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass",
                      line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.timeout(600)
def test_decode_kernels_fit_their_register_budget(tmp_path):
    r = subprocess.run(
        [HIPCC, "-c", SRC_ATTN, "-o", str(tmp_path / "k.o"),
         "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17",
         "-Rpass-analysis=kernel-resource-usage"],
        capture_output=True, text=True, timeout=560,
    )
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = resource_remarks(r.stderr)
    assert len(kernels) == N_KERNELS, len(kernels)
    spilled = [k for k, v in kernels.items()
               if (v["ScratchSize"], v["SGPRs Spill"], v["VGPRs Spill"])
               != ("0", "0", "0")]
    assert not spilled, spilled
    fused = {k: int(v["Occupancy"]) for k, v in kernels.items()
             if "attn_decode_fused_kernel" in k}
    assert len(fused) == 216, len(fused)
    low = {k: o for k, o in fused.items() if o < 4}
    assert not low, low
