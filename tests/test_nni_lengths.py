"""The host rules of the likelihood tree search (pansim_amd/csrc/nni_moves.h: the canonical form that carries branch lengths, the
selection over binary64 gains) against clade sets: tests/nni_lengths_check.cpp, a host program of its own (no device, nothing
loaded into Python), built with the address and undefined-behaviour sanitizers and run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lengths_follow_their_nodes_through_moves_and_canonical_forms(tmp_path):
    exe = str(tmp_path / "nni_lengths_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "nni_lengths_check.cpp")])
    # (leak checking needs ptrace, which a container may refuse; the program allocates nothing it keeps)
    run = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "every step matches" and not any("MISMATCH" in line for line in lines)
    assert lines[0].startswith("3600 steps, 720 batches of ") and int(lines[0].split()[-2]) > 720
