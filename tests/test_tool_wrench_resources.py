"""The tool-wrench kernels' resource usage, read from the built library's own code objects (tools/kernel_resources.py; no GPU,
no recompile): a point's whole state -- (w, wd, a) per evaluation; no accumulated rotation, the result is in link axes -- stays
in registers at any dof: no scratch, no vector or scalar register spills (the payload's 22 doubles are read from the argument
block after the loop over the links, not held across it), no static LDS (the dynamic LDS only stages a block's inputs and
outputs for contiguous global accesses), and at most the as-built register count plus 10 %, the convention of
tests/test_chain_resources.py and tests/test_tool_accel_resources.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# as built: registers (vector + accumulator), static LDS bytes per block (the staging area is dynamic LDS, sized by the launch)
AS_BUILT = {"chain_tool_wrench_kernel": (80, 0), "chain_tool_wrench_terms_kernel": (106, 0)}


@pytest.fixture(scope="module")
def kernels():
    import kernel_resources as kr
    from toppra_amd import build
    build.build()
    return {n: r for n, r in kr.kernels().items() if "chain_" in n}


@pytest.mark.parametrize("key", sorted(AS_BUILT))
def test_state_in_registers(kernels, key):
    regs, lds = AS_BUILT[key]
    rs = [r for n, r in kernels.items() if key in n]
    assert len(rs) == 1, (key, sorted(kernels))
    assert rs[0]["scratch"] == 0, (key, "scratch bytes per lane", rs[0]["scratch"])
    assert rs[0]["lds"] == lds, (key, "LDS bytes", rs[0]["lds"])
    assert rs[0]["vgpr"] <= int(1.1 * regs), (key, "registers", rs[0]["vgpr"], regs)
    assert rs[0]["vgpr_spill"] == 0 and rs[0]["sgpr_spill"] == 0, (key, rs[0])

