"""The LEAN evaluation's owner-tagged columns on the host (no GPU): scripts/lean_owner_check.cpp,
built with ASan / UBSan, holds the tagged container word to its states, capability-set id and owner
(all 2^15 state combinations, all 64 owners, ids 0 and 2047), the volume word to vol_code for no
source and each of the 29 single sources and to its escape flag for several sources, and a plain
C++ model of the scatter ("mask by the tile's count, OR into acc[owner]", with the next tile's
items in the slack slots) to cv_fails over the per-pod OR, through the packed class masks and pod
table. The functions are the ones the kernels and the host call (kyverno_amd/csrc/kernels_abi.h
kpe_l6_tag_*, cv_fails)."""
import subprocess

from tests.conftest import build_host_tool


def test_lean_owner_helpers_under_asan():
    tool = build_host_tool("lean_owner_check")
    res = subprocess.run([tool], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-2000:])
    assert "lean_owner_check ok" in res.stdout
