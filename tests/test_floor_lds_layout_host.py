"""The LDS layout of the floor forward kernels, replayed on the host: viterbi_spl_amd/csrc/floor_lds_check.hip is a stand-alone
program (its own main) that walks FloorLds' offset arithmetic for every instantiated (W, NWT), every win_shift and every window
start.  It is compiled for the host only, with the address and undefined-behaviour sanitizers, and run; no GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "viterbi_spl_amd", "csrc")


def test_floor_lds_offsets(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "floor_lds_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(CSRC, "floor_lds_check.hip")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "all checks passed" in out.stdout and "FAIL" not in out.stdout, out.stdout[-4000:]
    assert "FloorSplitLds" in out.stdout and "FloorLds<128, 12, Packed>" in out.stdout, out.stdout[-4000:]
