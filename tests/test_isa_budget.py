"""The rollout loop's static budget (tools/isa_budget.py: a cross-compile, no GPU): the path
sums stay at least 12 instructions under the counts of the code before the loops lost their
glue (148 for a one-block rollout that ends in a win, 191 with an absorbed fill), the
continuing block does not grow past its 166, and both product kernels keep 128 VGPRs without
scratch."""
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rollout_paths_registers_and_scratch(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_budget
    finally:
        sys.path.pop(0)
    asm = tmp_path / "c4_search.s"
    isa_budget.compile_asm(str(asm))
    out = io.StringIO()
    res = isa_budget.analyse(asm.read_text().splitlines(), out)
    print(out.getvalue())
    assert res["win"] <= 148 - 12
    assert res["absorbed"] <= 191 - 12
    assert res["continue"] <= 166
    for kernel in [isa_budget.KERNEL] + isa_budget.ALSO:
        vgprs, scratch = res[kernel]
        assert vgprs <= 128 and scratch == 0, kernel
