"""The split floor kernel's half-wave lane map (partner lanes l and l ^ 8, joined by one DPP maximum) and its frame-maximum slot map
with the extra column in M's quad of floats, replayed on the host by viterbi_spl_amd/csrc/floor_lds_check.hip: a stand-alone program
(its own main), compiled for the host only with the address and undefined-behaviour sanitizers, and run; no GPU.  This test holds the
lines the replay prints about the two maps and about the LDS cycles of the half waves' window reads."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "viterbi_spl_amd", "csrc")


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("floor_split_join") / "floor_lds_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(CSRC, "floor_lds_check.hip")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "all checks passed" in out.stdout and "FAIL" not in out.stdout, out.stdout[-4000:]
    return out.stdout


def test_lane_map_line(replay):
    assert "split lane map: partner l ^ 8 (row_ror:8), 32 lower lanes in ascending target order: ok" in replay


def test_slot_map_line(replay):
    m = re.search(r"split slot map: every quad without x reaches one of slots 0 \.\. 2, x reaches slot 3 alone: ok \((\d+) state counts\)", replay)
    assert m, replay[-2000:]
    assert int(m.group(1)) == 32              # S = 257, 261, .. 381: every state count with x = S - 1, x % 4 == 0 the split kernel takes


def test_window_read_cycles(replay):
    """Four ds_read_b128 of a half wave cost 16 LDS cycles without a bank conflict.  At the plan's own shift the new map may not be
    worse than the old one in any half wave; at the 361-state grid the old map's third half wave paid 24."""
    rows = re.findall(r"split window reads S (\d+) off (\d+) sh (\d)( \(the plan's\))?: ds_read_b128 cycles per half wave, halves 32 lanes apart "
                      r"(\d+) / (\d+) / (\d+) / (\d+), partner l \^ 8 (\d+) / (\d+) / (\d+) / (\d+)", replay)
    assert len(rows) == 8, replay[-3000:]
    plans = {}
    for S, off, sh, mark, *cyc in rows:
        cyc = [int(v) for v in cyc]
        assert all(v >= 16 for v in cyc)
        assert bool(mark) == (int(sh) == int(off) % 4)
        if mark:
            plans[int(S)] = (cyc[:4], cyc[4:])
    assert set(plans) == {361, 321}
    for S, (old, new) in plans.items():
        assert all(n <= o for n, o in zip(new, old)), (S, old, new)
    assert plans[361] == ([16, 16, 24, 16], [16, 16, 16, 16])
    assert plans[321][1] == [16, 16, 16, 16]
