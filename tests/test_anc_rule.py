"""The three functions pansim_amd/csrc/subst_rule.h adds for the marginal ancestral states (ps_subst_node_post, ps_subst_pdiff,
ps_subst_map; docs/ANCESTRAL_STATES.md) alone: tests/anc_rule_check.cpp, a host program of its own (no device, nothing loaded
into Python), built with the address and undefined-behaviour sanitizers and without fused multiply-adds, and run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_ancestral_rule_alone(tmp_path):
    exe = str(tmp_path / "anc_rule_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "anc_rule_check.cpp")])
    # (leak checking needs ptrace, which a container may refuse; the program allocates nothing it keeps)
    run = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "every step matches" and not any("MISMATCH" in line for line in lines)
    words = lines[-2].split()
    # posteriors, denormal sums that were not 0, differences with a likelihood, maps, and exact ties among them
    assert int(words[0]) == 20000 and int(words[2]) > 500 and int(words[5]) > 10000 and int(words[7]) == 20000 and int(words[10]) > 3000
