#!/usr/bin/env python
"""Record tests/golden/packed_weight_hashes.json: run every case of tests/pack_cases.py through the packers of cvvae_amd.ops on
the MI355X and store the hashes and PackedConv fields that tests/test_gpu_pack_bytes.py compares.

    python tools/record_pack_hashes.py --commit <the commit the loaded library was built from> [--out FILE]

Only a change that MEANS to alter the packed format re-records; a refactor of the packers must pass against the file as it is."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cvvae_amd import ops  # noqa: E402
from tests import pack_cases as PC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "packed_weight_hashes.json"))
    a = ap.parse_args()
    cases = {}
    for case, form in PC.params():
        pw, win = PC.run_case(ops, case, form)
        cases[f"{case.name}-{form}"] = PC.summarise(pw, win)
    with open(a.out, "w") as f:
        json.dump(dict(recorded_from=a.commit, cases=cases), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {a.out}")


if __name__ == "__main__":
    main()
