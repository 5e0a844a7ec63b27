"""The three-operation quotient of csrc/dev_math.inc (DevMathF::quot) pinned on the CPU, independently of any device:
tests/quotient_host.cpp restates it with fmaf and an emulated refined reciprocal (the correctly rounded reciprocal moved by
-1, 0, +1 units in the last place, then the Newton step) and compares it with `/` over the divisors and the structured
numerators of the device test (tests/test_gpu_quotient.py), wherever the refined reciprocal came out correctly rounded --
in a first pass over the operands of what = 3, in a second over div4's own operand box (what = 4): signed numerators at
exponent distances from -112 to +81, and the two zeros."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_three_operation_quotient_equals_division_given_an_exact_reciprocal(tmp_path):
    exe = str(tmp_path / "quotient_host")
    # (-ffp-contract=off: the program's own a*y1 must stay a rounded product, as in the library's build)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "quotient_host.cpp")])
    run = subprocess.run([exe, "1024"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert " 0 mismatches" in run.stdout, run.stdout
    box = [line for line in run.stdout.splitlines() if line.startswith("box: ")]
    assert len(box) == 1 and box[0].endswith(", 0 mismatches") and "pairs (" in box[0], run.stdout
