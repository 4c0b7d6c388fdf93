"""Which path lpr_primal_solve takes for given options on a given shape (csrc/primal_plan.hpp),
under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU: tools/primal_plan_check.cpp is a
stand-alone host program (its own main, no HIP, no GPU) that holds primal_plan() against a table of
expected plans written by hand from the documentation of lpr_solve_opts -- path, pivots per sweep
and tile for every shape threshold, every value of block and variant the header names, every flag
bit, the condensed-layout rules and the spare-column rule.  Every path stores the same bits, so no
other test would notice a wrong decision."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_table_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "primal_plan_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "primal_plan_check.cpp"),
                    "-o", exe], check=True, capture_output=True, timeout=300)
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    tail = (proc.stdout + proc.stderr)[-3000:]
    assert proc.returncode == 0, tail
    assert " 0 failures" in proc.stdout and "runtime error" not in tail, tail
