"""The sensitivity report's workspace layout and tile geometry (csrc/sens_ranging_common.hpp) under
AddressSanitizer + UndefinedBehaviorSanitizer on the CPU: tools/ranging_plan_check.cpp is a
stand-alone host program (its own main, no HIP, no GPU) that walks every index the two kernels form
over exactly-sized buffers, checks that every slab cell is written exactly once and that shapes
with n < 0 are refused."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_and_indices_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ranging_plan_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "ranging_plan_check.cpp"),
                    "-o", exe], check=True, capture_output=True, timeout=300)
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    tail = (proc.stdout + proc.stderr)[-3000:]
    assert proc.returncode == 0, tail
    assert " 0 failures" in proc.stdout and "runtime error" not in tail, tail
