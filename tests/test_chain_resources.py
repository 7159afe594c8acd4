"""The chain kernels' resource usage, read from the built library's own code objects (tools/kernel_resources.py; no GPU, no
recompile): the 1..8-dof instantiations keep a point's whole state in registers -- NO scratch -- and every kernel stays under
its committed ceilings, the as-built values plus 10 %.

Why this is a test: the fused 8-dof kernel holds 17 doubles per link and evaluation set next to its working values, 371 of the
512 registers a lane can have.  Two value-identical spellings cost 420 - 1476 bytes of scratch per lane while it was written:
the fully unrolled links without fences between them (the scheduler starts every link's sines and parameter loads at once), and
a store of the outputs under a condition (it draws the whole backward pass into its branch, past the fences)."""
import os
import re

import pytest

from tests.resource_support import built_kernels, val

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# as built: registers (vector + accumulator) and static LDS bytes per block, per dof
SINGLE = {1: (44, 1536), 2: (87, 4608), 3: (104, 4608), 4: (123, 7680), 5: (142, 7680), 6: (162, 10752), 7: (181, 10752), 8: (204, 13824)}
FUSED = {1: (74, 1536), 2: (138, 4608), 3: (214, 4608), 4: (282, 7680), 5: (288, 7680), 6: (309, 10752), 7: (327, 10752), 8: (371, 13824)}
# the runtime-dof kernels (9..32 dof: state in dynamic LDS, sized by the launch) and the tool velocity kernel: registers
RUNTIME = {"chain_inverse_dynamics_lds_kernel": 95, "chain_torque_terms_lds_kernelILb1E": 121, "chain_torque_terms_lds_kernelILb0E": 135,
           "chain_tool_velocity_kernel": 96}


@pytest.fixture(scope="module")
def kernels():
    return built_kernels("chain_")


@pytest.mark.parametrize("kernel,table", [("chain_inverse_dynamics_kernel", SINGLE), ("chain_torque_terms_kernel", FUSED)])
def test_register_resident_kernels_use_no_scratch(kernels, kernel, table):
    found = {}
    for name, r in kernels.items():
        m = re.search(kernel + r"ILi(\d+)E", name)
        if m:
            found[int(m.group(1))] = r
    assert sorted(found) == list(range(1, 9)), sorted(found)
    for d, r in sorted(found.items()):
        regs, lds = table[d]
        assert r["scratch"] == 0, (kernel, d, "scratch bytes per lane", r["scratch"])
        assert r["vgpr"] <= min(512, int(1.1 * regs)), (kernel, d, "registers", r["vgpr"], regs)
        assert r["lds"] <= int(1.1 * lds), (kernel, d, "LDS bytes", r["lds"], lds)


def test_runtime_dof_kernels(kernels):
    for key, regs in RUNTIME.items():
        rs = [r for n, r in kernels.items() if key in n]
        assert len(rs) == 1, (key, sorted(kernels))
        assert rs[0]["scratch"] == 0 and rs[0]["lds"] == 0, (key, rs[0])  # (their LDS is dynamic: at most 160 KB, checked at launch)
        assert rs[0]["vgpr"] <= int(1.1 * regs), (key, rs[0]["vgpr"], regs)


def test_the_launch_s_lds_fits_the_cu():
    """d * slots * 64 lanes * 8 bytes: the single evaluation fits 160 KB up to 32 dof, the fused state up to 18 dof (the
    launcher switches to one evaluation after the other above), as csrc/tpr_chain_args.hpp states it."""
    text = open(os.path.join(ROOT, "toppra_amd", "csrc", "tpr_chain_args.hpp")).read()
    single, fused = val("kChainSlotsSingle", text), val("kChainSlotsFused", text)
    assert (single, fused) == (8, 17)
    assert 32 * single * 64 * 8 <= 160 * 1024
    assert 18 * fused * 64 * 8 <= 160 * 1024 < 19 * fused * 64 * 8
