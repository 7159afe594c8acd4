"""The control-point kernels' resource usage, read from the built library's own code objects (tools/kernel_resources.py; no GPU,
no recompile): a path point's whole state -- (v, w) or (w, wd, a) per evaluation and the accumulated rotation W -- stays in
registers at any dof and for any point set: no scratch, no spills, no static LDS (the dynamic LDS only stages a block's inputs
and holds its outputs for contiguous global accesses), and at most the as-built register count plus 10 %, the convention of
tests/test_chain_resources.py.  The dynamic LDS is checked against the 64 KB a kernel may take without asking."""
import os
import re

import pytest

from tests.resource_support import built_kernels, in_registers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# as built: registers (vector + accumulator), static LDS bytes per block
AS_BUILT = {"chain_points_speed_kernel": (124, 0), "chain_points_accel_kernel": (126, 0), "chain_points_accel_terms_kernel": (138, 0)}


@pytest.fixture(scope="module")
def kernels():
    return built_kernels("chain_")


@pytest.mark.parametrize("key", sorted(AS_BUILT))
def test_state_in_registers(kernels, key):
    regs, lds = AS_BUILT[key]
    rs = [r for n, r in kernels.items() if key in n]
    assert len(rs) == 1, (key, sorted(kernels))
    in_registers(rs[0], regs, key, static_lds=lds)


def test_the_new_names_leave_the_older_tests_their_kernels(kernels):
    """The resource tests of the tool kernels pick a kernel by a substring of its name and expect one match."""
    for key in ("chain_tool_velocity_kernel", "chain_tool_accel_kernel", "chain_tool_accel_terms_kernel", "chain_tool_wrench_kernel",
                "chain_tool_wrench_terms_kernel", "chain_inverse_dynamics_lds_kernel"):
        assert len([n for n in kernels if key in n]) == 1, key
        assert not [n for n in kernels if key in n and "points" in n], key


def test_the_dynamic_lds_needs_no_permission():
    """The inputs of three links at pitch 3 beside the outputs at pitch 3 P | 1 (csrc/tpr_chain.hip.inc: chain_points_lds_bytes; the
    two cannot share their space: a point's output exists from its link on, while the deeper links' inputs are still to be read).
    The size does not depend on the dof: at most 54 784 bytes over P = 1..16 for both kernels, under the 64 KB of dynamic LDS a
    launch gets without an attribute."""
    text = open(os.path.join(ROOT, "toppra_amd", "csrc", "tpr_chain.hip.inc")).read()
    assert ("return (3 * (size_t)kChainBlock * (size_t)kChainPointsChunk + (size_t)outputs * kChainBlock * (size_t)(3 * count | 1)) * sizeof(double);"
            in text)
    args = open(os.path.join(ROOT, "toppra_amd", "csrc", "tpr_chain_args.hpp")).read()
    assert re.search(r"constexpr int kChainBlock = 64;", args)
    chunk = int(re.search(r"constexpr int kChainPointsChunk = (\d+);", args).group(1))
    assert chunk % 2 == 1  # (the staging pitch: odd, or the rows' reads conflict)
    size = lambda count, outputs: (3 * 64 * chunk + outputs * 64 * (3 * count | 1)) * 8  # noqa: E731
    assert max(size(P, o) for P in range(1, 17) for o in (1, 2)) == size(16, 2) == 3 * 64 * chunk * 8 + 50176 <= 64 * 1024
    assert chunk == 3 and size(16, 2) == 54784 and size(4, 2) == 17920
