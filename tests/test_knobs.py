"""The weight gradient's environment knobs have ONE table (cvvae_amd/csrc/knobs.h):
  * wgrad_kernel.hip reads the environment through it only;
  * the knob paragraph of tools/README.md names every knob of the table;
  * every weight-gradient knob a test or a tool sets is in the table;
  * the read-once policy holds: a knob set in a child process's environment changes that process's selection or sizes (a knob set
    after the first use would change nothing: that is why those variants of tests/conv_selection_cases.py run in children).
The forward convolution's knobs (CVVAE_CONV_*) are still read in cvvae_api.hip and conv_kernel.h; their variants are checked for the
same liveness here, so that the record they are compared with (tests/test_conv_selection_parity.py) means something."""
import glob
import os
import re

import pytest

from tests import conv_selection_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cvvae_amd", "csrc")
KNOBS_H = os.path.join(CSRC, "knobs.h")
RULES = {"INT", "REAL", "NONZERO", "PRESENT", "TEXT"}


def table():
    """{name: (rule, default, read)} parsed from the rows of CVVAE_KNOBS"""
    text = open(KNOBS_H).read()
    body = text[text.index("#define CVVAE_KNOBS(X)"):text.index("enum KnobRule")]
    rows = re.findall(r'X\((\w+),\s*"(CVVAE_\w+)",\s*(\w+),\s*([-\w.]+),\s*(ONCE|PER_CALL),', body)
    assert len(rows) == body.count("\n  X(")  # (every row parsed)
    assert all("CVVAE_" + i == n and r in RULES for i, n, r, _, _ in rows)
    return {n: (r, d, p) for _, n, r, d, p in rows}


def test_the_table_holds_the_weight_gradients_knobs_and_their_read_policies():
    t = table()
    assert {n: v[2] for n, v in t.items()} == {"CVVAE_WGRAD_DMA": "ONCE", "CVVAE_WGRAD_WGS": "ONCE", "CVVAE_WGRAD_FAST": "PER_CALL"}


def test_the_weight_gradient_reads_the_environment_through_the_table_only():
    assert "getenv" not in open(os.path.join(CSRC, "wgrad_kernel.hip")).read()
    assert "getenv" in open(KNOBS_H).read()


def test_the_readme_paragraph_names_the_tables_knobs():
    text = open(os.path.join(ROOT, "tools", "README.md")).read()
    start = text.index("Library knobs (")
    para = text[start:text.index("\n\n", start)]
    assert set(table()) <= set(re.findall(r"`(CVVAE_[A-Z0-9_]+)", para))


def test_every_weight_gradient_knob_the_tests_and_tools_set_is_in_the_table():
    pat = re.compile(r"\bCVVAE_WGRAD_[A-Z0-9_]*[A-Z0-9]\b")
    files = glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "**", "*.py"), recursive=True)
    used = set()
    for f in files:
        used |= set(pat.findall(open(f).read()))
    assert {"CVVAE_WGRAD_DMA", "CVVAE_WGRAD_FAST"} <= used  # (the scan finds them)
    assert used <= set(table()), sorted(used - set(table()))


@pytest.mark.parametrize("name,corpus", [(n, c) for n, e, c in SC.VARIANTS if e])
def test_a_knob_in_the_environment_changes_the_selection(name, corpus):
    rec = SC.recorded()[corpus]
    changed = sum(a != b for fam in rec["default"] for a, b in zip(rec["default"][fam], rec[name][fam]))
    assert changed > 0, f"{name}: no row of the {corpus} corpus differs from the default; add one that does"
