"""csrc/dev_owner.hpp -- the owners of device buffers, events, ordering marks, streams and page-locked blocks that trmc_plan and
StreamRun are made of -- checked on the CPU: tests/dev_owner_host.cpp compiles the header against counting stand-ins for the HIP
calls it makes, with the address and undefined-behaviour sanitizers, and runs as a program of its own.  It is the library's leak
check: every case (growth, a failing allocation, moves, vectors that reallocate, swap, an early return, events made once, a block
shared by three holders destroyed in all six orders; and an ordering mark's: record, order two streams, settle; no call while
nothing is pending; a failing wait settles; a failing creation; moves; one event per mark) must release exactly what it made, once."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owners_release_what_they_hold_exactly_once(tmp_path):
    exe = str(tmp_path / "dev_owner_host")
    # (the sanitizers' runtimes linked INTO the program: it then starts in any environment, whatever that preloads)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "dev_owner_host.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert run.stdout.count(" ok") == 14 and "FAILED" not in run.stdout, run.stdout
