"""pansim_amd/csrc/gene_rule.h, the arithmetic of the gene gain / loss model (docs/GENE_MODEL.md), alone:
tests/gene_rule_check.cpp, a host program of its own (no device, nothing loaded into Python), built with the address and
undefined-behaviour sanitizers and without fused multiply-adds, and run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_gene_rule_alone(tmp_path):
    exe = str(tmp_path / "gene_rule_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "gene_rule_check.cpp")])
    # (leak checking needs ptrace, which a container may refuse; the program allocates nothing it keeps)
    run = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "every step matches" and not any("MISMATCH" in line for line in lines)
    words = lines[-2].split()
    # messages, joins, posteriors with exact ties among them, denormal sums that were not 0, joints and those with a likelihood
    assert int(words[0]) == 20000 and int(words[2]) == 20000 and int(words[4]) == 20000 and int(words[7]) >= 4000
    assert int(words[9]) > 500 and int(words[12]) == 20000 and int(words[14]) > 10000
