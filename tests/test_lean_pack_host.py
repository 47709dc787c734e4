"""The LEAN evaluation's compact container word and packed evidence numbering on the host (no GPU):
scripts/lean_pack_check.cpp, built with ASan / UBSan, holds the container word to its unpack for
all 2^15 used-state combinations (unused CX_* bits set and clear, capability-set ids 0, 1, 2046,
2047, never 0, bit 31 set), the packed numbering to a permutation of the in-place one, and the
packed class masks and pod table to cv_fails for every versioned check. The functions are the
ones the kernels and the host call (kyverno_amd/csrc/kernels_abi.h kpe_l6_pack_*, cv_fails)."""
import subprocess

from tests.conftest import build_host_tool


def test_lean_pack_helpers_under_asan():
    tool = build_host_tool("lean_pack_check")
    res = subprocess.run([tool], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-2000:])
    assert "lean_pack_check ok" in res.stdout
