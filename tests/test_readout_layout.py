"""The scratch layouts of the device read-outs against their first offset arithmetic: tests/readout_layout_check.cpp, a host
program of its own (no device, nothing loaded into Python), built with the address and undefined-behaviour sanitizers and run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layouts_match_the_first_offset_arithmetic(tmp_path):
    exe = str(tmp_path / "readout_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "readout_layout_check.cpp")])
    # (leak checking needs ptrace, which a container may refuse; the program allocates nothing it keeps)
    run = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "every layout matches" and not any("MISMATCH" in line for line in lines)
    # six sizes x (clusters, 2 trees, 6 neighbour lists, 2 genealogies, 4 ld parts)
    assert len(lines) == 6 * 15 + 1
