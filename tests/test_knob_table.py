"""The environment knobs and build defines stay listed: the BCHK_* names the library reads
through csrc/bchk_env.h are the rows of DESIGN.md's knob table, and every -DBCHK_* of the two
Makefiles names a macro that csrc/ tests. Text files only."""
import glob
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "polar-codes-with-bch-kernel_amd")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _csrc():
    return {p: _read(p) for p in sorted(glob.glob(os.path.join(PKG, "csrc", "*")))}


def test_knob_table_matches_the_helpers():
    src = _csrc()
    assert src
    read = set()
    for path, text in src.items():
        read |= set(re.findall(r'\benv_(?:flag|bool|int|u64|double)\(\s*"(BCHK_[A-Z0-9_]+)"', text))
        if os.path.basename(path) != "bchk_env.h":  # no BCHK_* variable read past the helpers
            assert not re.search(r'getenv\(\s*"BCHK_', text), path
    design = _read(os.path.join(REPO, "DESIGN.md"))
    section = design.split("#### Environment knobs", 1)[1].split("\n## ", 1)[0]
    table = set(re.findall(r"^\| `(BCHK_[A-Z0-9_]+)` \|", section, flags=re.M))
    assert len(read) > 30
    assert read == table, (sorted(read - table), sorted(table - read))


def test_makefile_defines_name_tested_macros():
    tested = set()
    for text in _csrc().values():
        for line in re.findall(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$", text, flags=re.M):
            tested |= set(re.findall(r"\bBCHK_[A-Z0-9_]+\b", line))
    defined = set()
    for mk in ("Makefile", "Makefile.experiments"):
        defined |= set(re.findall(r"-D(BCHK_[A-Z0-9_]+)", _read(os.path.join(PKG, mk))))
    assert {"BCHK_DIAG", "BCHK_AN_PROF", "BCHK_FP_TRACE"} <= defined
    assert defined <= tested, sorted(defined - tested)
