"""What the resource tests of the rigid-body kernels share (tests/test_chain_resources.py, _tree, _tool_accel, _tool_wrench,
_control_points, _base_wrench, _joint_load, _momentum): the built library's kernels, the "state in registers" check and the
reader of a constant in the sources.  A plain module: each test file keeps its own constants and LDS arithmetic."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def built_kernels(containing=""):
    """{kernel name: resources} of the library as built (tools/kernel_resources.py; no GPU, no recompile), the names that
    contain ``containing``."""
    import kernel_resources as kr
    from toppra_amd import build
    build.build()
    return {n: r for n, r in kr.kernels().items() if containing in n}


def in_registers(r, as_built, what=None, static_lds=0, parked_scalars=False):
    """A kernel's whole state stays in registers: no scratch, no vector or scalar register spills, no static LDS (but
    ``static_lds`` bytes as built; the dynamic LDS is sized by the launch), no accumulator registers, and at most the as-built
    count of vector registers plus 10 %.  ``parked_scalars``: the compiler may park scalar registers in lanes of a vector
    register across the loops, which costs no memory traffic -- what the tree walk's kernels are built with."""
    assert r["scratch"] == 0, (what, "scratch bytes per lane", r["scratch"])
    assert r["vgpr_spill"] == 0 and (parked_scalars or r["sgpr_spill"] == 0), (what, r)
    assert r["lds"] == static_lds, (what, "static LDS bytes", r["lds"])
    assert r["agpr"] == 0 and r["vgpr"] <= int(1.1 * as_built), (what, "registers", r["vgpr"], as_built)


def val(name, text):
    """The integer constant ``name = a + b + ...`` of a source text."""
    return sum(int(x) for x in re.search(name + r" = ([0-9+ ]+)[,;]", text).group(1).split("+"))
