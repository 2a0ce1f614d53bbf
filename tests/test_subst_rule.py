"""The arithmetic of the likelihood under F81 with a root distribution and rate categories (pansim_amd/csrc/subst_rule.h: the
messages, the mixture, the posterior, the derivative ratios and terms, the Newton step, the start lengths) against the sum over
all assignments, and its JC69 anchor bit for bit against jc_rule.h: tests/subst_rule_check.cpp, a host program of its own (no
device, nothing loaded into Python), built with the address and undefined-behaviour sanitizers and without fused multiply-adds,
and run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rule_header_alone(tmp_path):
    exe = str(tmp_path / "subst_rule_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "subst_rule_check.cpp")])
    # (leak checking needs ptrace, which a container may refuse; the program allocates nothing it keeps)
    run = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "every step matches" and not any("MISMATCH" in line for line in lines)
    words = lines[0].split()
    assert words[0] == "3000" and words[1] == "trees," and int(words[4]) > 1000 and int(words[6]) > 1000     # mixtures, anchored ratios
