"""The flush section of tools/isa_budget.py (a cross-compile, no GPU): a level of the prefetching
walk is decided in fp32 — its common path holds at most the one fp64 instruction that converts
log N — and costs fewer instructions than the fp64 level did (125); the fp64 scores are still
in the loop as the fallback."""
import io
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walk_level_is_fp32_with_an_fp64_fallback(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_budget
    finally:
        sys.path.pop(0)
    asm = tmp_path / "c4_search.s"
    isa_budget.compile_asm(str(asm))
    out = io.StringIO()
    res = isa_budget.analyse(asm.read_text().splitlines(), out)
    text = out.getvalue()
    print(text)
    flush = res["flush"]
    assert flush["walk level, fp32 decision"] < 125
    assert "walk level, fp64 scores" in flush
    fast = next(l for l in text.splitlines() if l.startswith("flush walk level, fp32 decision"))
    assert int(re.search(r"\(fp64 (\d+)\)", fast).group(1)) <= 1
