"""Every answer of the `pansim` executable that comes before any device work -- clap's errors (status 2), values that do
not parse and the extensions' flag checks (status 101), the validation messages (stdout, status 0), the help texts --
compared in full with tests/golden/cli_messages.json: exit status, stdout and stderr.  The cases with two faulty flags pin
the order in which the flags are checked.  The fixture was recorded by tests/golden/make_cli_messages.py from the
executable of the commit before the read-outs moved to cli_readouts.h; none of its cases reaches the library's device
check, so the answers are the same with and without a GPU."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "pansim_amd", "pansim")
CASES = json.load(open(os.path.join(HERE, "golden", "cli_messages.json")))


def test_the_table_covers_the_kinds_of_answer():
    assert {c["returncode"] for c in CASES} == {0, 2, 101}
    assert any(c["args"] == ["--help-extensions"] and "MI355X OPTIONS" in c["stdout"] for c in CASES)
    assert any(c["returncode"] == 0 and c["stdout"].startswith("pop_size, core_size") for c in CASES)
    assert not any("HIP device" in c["stderr"] for c in CASES)
    assert len({tuple(c["args"]) for c in CASES}) == len(CASES) >= 100


@pytest.fixture(scope="module")
def exe(pa):
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()
    return EXE


@pytest.mark.parametrize("case", CASES, ids=[" ".join(c["args"]) or "-" for c in CASES])
def test_answer_is_the_recorded_one(exe, tmp_path, case):
    r = subprocess.run([exe, *case["args"]], capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert (r.returncode, r.stdout, r.stderr) == (case["returncode"], case["stdout"], case["stderr"])
    assert os.listdir(tmp_path) == []
