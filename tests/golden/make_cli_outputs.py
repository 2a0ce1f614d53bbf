#!/usr/bin/env python3
"""Record tests/golden/cli_outputs.json: every file the `pansim` executable writes for the three runs of
tests/test_gpu_cli_outputs.py (its command line and its runs are used as they stand there).  Run on an MI355X with the
executable of the commit BEFORE a change of the command line's code, built in a scratch checkout:
    python tests/golden/make_cli_outputs.py /path/to/that/checkout/pansim_amd/pansim
Everything is run twice.  The two recordings must agree, and so must the runs on one and on two shards; the resumed run
may differ from the uninterrupted one only in the files that depend on the genealogy record, and only those are kept
for it.  A file that differs between the two recordings is a finding: it is named, and the script refuses to write."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_gpu_cli_outputs as t  # noqa: E402

if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    exe = os.path.abspath(sys.argv[1])
    rec = []
    for k in range(2):
        with tempfile.TemporaryDirectory() as tmp:
            rec.append({form: t.run_form(exe, form, os.path.join(tmp, "r%d" % k)) for form in ("gpus1", "gpus2", "resume")})
    unstable = sorted({(form, s) for form in rec[0] for s in set(rec[0][form]) | set(rec[1][form])
                       if rec[0][form].get(s) != rec[1][form].get(s)})
    if unstable:
        sys.exit("two recordings differ in %s" % unstable)
    full, resume = rec[0]["gpus1"], rec[0]["resume"]
    shards = sorted(s for s in set(full) | set(rec[0]["gpus2"]) if full.get(s) != rec[0]["gpus2"].get(s))
    if shards:
        sys.exit("one and two shards differ in %s" % shards)
    differs = {s for s in set(full) | set(resume) if full.get(s) != resume.get(s)}
    if not differs <= t.RECORD_DEPENDENT:
        sys.exit("the resumed run differs from the uninterrupted one in %s" % sorted(differs - t.RECORD_DEPENDENT))
    with open(t.GOLDEN, "w") as f:
        json.dump({"full": {s: t.pack(full[s]) for s in full}, "resume": {s: t.pack(resume[s]) for s in differs}}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d files of the full run (%d bytes), %d of the resumed one: %s" % (len(full), sum(map(len, full.values())), len(differs), sorted(differs)))
    print(full["_clusters_summary.tsv"] + full["_diff_groups.tsv"] + full["(stderr)"])
