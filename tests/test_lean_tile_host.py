"""kpe_lean6_kernel's tile-body helpers on the host (no GPU): scripts/lean_tile_check.cpp, built
with ASan / UBSan, holds the pod-evidence table to the field logic for every pod word, the
four-word container read to a loop over the pod's slots, and the class masks to the one-check
rule. The helpers are the functions the kernel calls (kyverno_amd/csrc/kernels_abi.h kpe_l6_*)."""
import subprocess

from tests.conftest import build_host_tool


def test_lean_tile_helpers_under_asan():
    tool = build_host_tool("lean_tile_check")
    res = subprocess.run([tool], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-2000:])
    assert "lean_tile_check ok" in res.stdout
