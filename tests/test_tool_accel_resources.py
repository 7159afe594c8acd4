"""The tool-acceleration kernels' resource usage, read from the built library's own code objects (tools/kernel_resources.py;
no GPU, no recompile): a point's whole state -- (w, wd, a) per evaluation and the accumulated rotation W -- stays in
registers at any dof: no scratch, no static LDS (the dynamic LDS only stages a block's inputs and outputs for contiguous
global accesses), and at most the as-built register count plus 10 %, the convention of tests/test_chain_resources.py.  The
staging area's size is checked against the 64 KB a kernel may take without asking."""
import os

import pytest

from tests.resource_support import built_kernels, in_registers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# as built: registers (vector + accumulator), static LDS bytes per block (the staging area is dynamic LDS, sized by the launch)
AS_BUILT = {"chain_tool_accel_kernel": (98, 0), "chain_tool_accel_terms_kernel": (118, 0)}


@pytest.fixture(scope="module")
def kernels():
    return built_kernels("chain_")


@pytest.mark.parametrize("key", sorted(AS_BUILT))
def test_state_in_registers(kernels, key):
    regs, lds = AS_BUILT[key]
    rs = [r for n, r in kernels.items() if key in n]
    assert len(rs) == 1, (key, sorted(kernels))
    in_registers(rs[0], regs, key, static_lds=lds)


def test_the_staging_area_needs_no_permission():
    """3 arrays x 64 rows x (d | 1) doubles, or the outputs at pitch 7 where that is more (csrc/tpr_chain.hip.inc:
    chain_accel_lds_bytes): at most 50 688 bytes at 32 dof, under the 64 KB of dynamic LDS a launch gets without an attribute."""
    text = open(os.path.join(ROOT, "toppra_amd", "csrc", "tpr_chain.hip.inc")).read()
    assert "in = 3 * (size_t)kChainBlock * (size_t)(d | 1), out = (size_t)outputs * kChainBlock * 7" in text
    size = lambda d, outputs: max(3 * 64 * (d | 1), outputs * 64 * 7) * 8  # noqa: E731
    assert max(size(d, o) for d in range(1, 33) for o in (1, 2)) == 50688 <= 64 * 1024
    assert size(1, 2) == 2 * 64 * 7 * 8  # (at 1 .. 3 dof the fused kernel's outputs are the larger part)
