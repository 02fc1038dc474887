"""CPU: the table of environment switches in INTEGRATION.md (section "Environment switches of the library") is the list of
TPG_* variables the library and the R shim read -- no row for a variable nothing reads, no variable without a row."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# getenv("TPG_X") and the two helpers of csrc/common.h, tpg_env_set("TPG_X") / tpg_env_int("TPG_X", dflt)
READ = re.compile(r'\b(?:getenv|tpg_env_set|tpg_env_int)\s*\(\s*"(TPG_[A-Z0-9_]+)"')
NAME = re.compile(r"TPG_[A-Z0-9_]+")
# rows the table itself marks as not the library's: read by bench.py only, or by the tests' own code only
NOT_THE_LIBRARYS = re.compile(r"read by `bench\.py` only|of the tests only")


# a string literal, or a comment: comments are dropped, so that a name in a stale comment keeps no row alive
_LITERAL_OR_COMMENT = re.compile(r'"(?:\\.|[^"\\\n])*"|//[^\n]*|/\*.*?\*/', re.S)


def _sources():
    """(path relative to the repository, text without comments) of every source file of the library and of the shim"""
    files = [p for p in glob.glob(os.path.join(ROOT, "tidypopgen_amd", "csrc", "**", "*"), recursive=True)
             if p.endswith((".hip", ".h", ".c", ".cpp"))]
    files.append(os.path.join(ROOT, "shim", "tpg_rshim.c"))
    assert len(files) > 10
    for p in files:
        with open(p, encoding="utf-8") as f:
            text = _LITERAL_OR_COMMENT.sub(lambda m: m.group(0) if m.group(0).startswith('"') else " ", f.read())
        yield os.path.relpath(p, ROOT), text


def _names_read():
    names = {}
    for p, text in _sources():
        for nm in READ.findall(text):
            names.setdefault(nm, p)
    return names


def _names_in_table():
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as f:
        text = f.read()
    section = text.split("## 6. Environment switches of the library", 1)[1]
    rows = [ln for ln in section.splitlines() if ln.startswith("|")]
    assert rows[0].replace(" ", "") == "|variable|effect|" and set(rows[1]) <= set("|-")
    names = set()
    for ln in rows[2:]:
        first, effect = ln.strip("|").split("|", 1)
        if not NOT_THE_LIBRARYS.search(effect):
            names.update(NAME.findall(first))
    return names


def test_every_switch_the_library_reads_has_a_row_and_every_row_a_reader():
    read, table = _names_read(), _names_in_table()
    assert len(read) > 30  # (the patterns still find the call sites)
    undocumented = {nm: where for nm, where in read.items() if nm not in table}
    assert not undocumented, f"read by the sources, no row in INTEGRATION.md: {undocumented}"
    stale = sorted(table - set(read))
    assert not stale, f"rows of INTEGRATION.md for variables nothing reads: {stale}"


def test_no_environment_read_hides_behind_a_computed_name():
    """Every getenv / tpg_env_* call of the library takes a string literal (common.h's two helpers pass their parameter on),
    so the scan above sees every name."""
    call = re.compile(r"\b(getenv|tpg_env_set|tpg_env_int)\s*\(\s*([^)\s,]+)")
    for p, text in _sources():
        for fn, arg in call.findall(text):
            if os.path.basename(p) == "common.h" and arg in ("name", "const"):
                continue  # the helpers' own definitions
            assert arg.startswith('"'), f"{p}: {fn}({arg} ...)"
