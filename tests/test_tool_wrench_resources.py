"""The tool-wrench kernels' resource usage, read from the built library's own code objects (tools/kernel_resources.py; no GPU,
no recompile): a point's whole state -- (w, wd, a) per evaluation; no accumulated rotation, the result is in link axes -- stays
in registers at any dof: no scratch, no vector or scalar register spills (the payload's 22 doubles are read from the argument
block after the loop over the links, not held across it), no static LDS (the dynamic LDS only stages a block's inputs and
outputs for contiguous global accesses), and at most the as-built register count plus 10 %, the convention of
tests/test_chain_resources.py and tests/test_tool_accel_resources.py."""
import os

import pytest

from tests.resource_support import built_kernels, in_registers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# as built: registers (vector + accumulator), static LDS bytes per block (the staging area is dynamic LDS, sized by the launch)
AS_BUILT = {"chain_tool_wrench_kernel": (80, 0), "chain_tool_wrench_terms_kernel": (106, 0)}


@pytest.fixture(scope="module")
def kernels():
    return built_kernels("chain_")


@pytest.mark.parametrize("key", sorted(AS_BUILT))
def test_state_in_registers(kernels, key):
    regs, lds = AS_BUILT[key]
    rs = [r for n, r in kernels.items() if key in n]
    assert len(rs) == 1, (key, sorted(kernels))
    in_registers(rs[0], regs, key, static_lds=lds)

