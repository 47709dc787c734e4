"""The LEAN evaluation's pod word column pw4 on the host (no GPU): scripts/lean_narrow_check.cpp,
built with ASan / UBSan, holds the one-word pod record of the narrow scatter form to what the rec12
form reads of a pod record, for every x in 0 .. 2^23 - 1 and the kind ids 0, 1, 511 and 1023: the
narrow table lookup equals kpe_l6_pod_lookup of x, the class, the decode error and the kind id come
back, and neither bits 23-31 of x nor the version / group bits of y leak in. The functions are the
ones the kernels and the host call (kyverno_amd/csrc/kernels_abi.h kpe_l6_pack_pod, kpe_l6p_*)."""
import subprocess

from tests.conftest import build_host_tool


def test_lean_narrow_helpers_under_asan():
    tool = build_host_tool("lean_narrow_check")
    res = subprocess.run([tool], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-2000:])
    assert "lean_narrow_check ok" in res.stdout
