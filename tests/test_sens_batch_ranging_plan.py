"""The LDS carve-up, the output layout and the lane mapping of the scenario batch's sensitivity
report (csrc/sens_batch_ranging_common.hpp) under AddressSanitizer + UndefinedBehaviorSanitizer on
the CPU: tools/sens_batch_ranging_check.cpp is a stand-alone host program (its own main, no HIP, no
GPU) that walks every index k_sens_batch_ranging forms over exactly-sized buffers -- fixed-shape
and grow batches -- and checks that every output cell, the padding included, is written exactly
once, that every row is owned by one wave and every column of a row by one lane, ascending."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_and_indices_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sens_batch_ranging_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "sens_batch_ranging_check.cpp"),
                    "-o", exe], check=True, capture_output=True, timeout=300)
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    tail = (proc.stdout + proc.stderr)[-3000:]
    assert proc.returncode == 0, tail
    assert " 0 failures" in proc.stdout and "runtime error" not in tail, tail
