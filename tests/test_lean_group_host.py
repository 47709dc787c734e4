"""The group form of the LEAN evaluation's scatter on the host (no GPU): scripts/lean_group_check.cpp,
built with ASan / UBSan, holds the item words that carry a quarter (the pod's tile within its group
of four) to their owner, quarter, id and slot for all quarters and owners, the builders without a
quarter to quarter 0 and their earlier owners, and a lane-by-lane model of the group scatter (256
interleaved words per wave, the lists streamed from the group's first item to its last in 64-slot
sets, masked by the group's count) to the per-tile model and to each pod's own items, over
hand-built corpora: a clean group followed at once by the next group's offending items in every
list, last groups of fewer than four tiles, tiles with no item of a list, and groups with more items
than the sets loaded up front. The functions are the ones the kernels and the host call
(kyverno_amd/csrc/kernels_abi.h kpe_l6_tag_*)."""
import subprocess

from tests.conftest import build_host_tool


def test_lean_group_model_under_asan():
    tool = build_host_tool("lean_group_check")
    res = subprocess.run([tool], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-2000:])
    assert "lean_group_check ok" in res.stdout
