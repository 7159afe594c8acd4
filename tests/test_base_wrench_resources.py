"""The base-reaction kernels' resource usage, read from the built library's own code objects (tools/kernel_resources.py; no GPU,
no recompile): exactly two kernels answer to "mount_wrench" and none of them to the names the chain and tree tests pick their
kernels by; a point's whole state -- W, p, the weight's sums, (w, wd, a) and the dynamic sums (f, n) per evaluation -- stays in registers at any dof: no
scratch, no vector or scalar register spills (the mount's 16 doubles and the walk's byte tables are read from the argument block
where they are needed, and a link's parameters are fetched in two parts), no static LDS (the dynamic LDS stages a block's inputs
and outputs and keeps the forks' banks), at most the as-built register count plus 10 %, and the launch's LDS arithmetic."""
import os
import re

import pytest

from tests.resource_support import built_kernels, in_registers, val

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# as built: registers (vector + accumulator)
AS_BUILT = {"mount_wrench_kernel": 134, "mount_wrench_terms_kernel": 162}


@pytest.fixture(scope="module")
def kernels():
    return built_kernels()


def test_exactly_two_mount_kernels(kernels):
    mine = sorted(n for n in kernels if "mount_wrench" in n)
    assert len(mine) == 2, mine
    for key in AS_BUILT:
        assert sum(key in n for n in mine) == 1, (key, mine)
    # the chain and tree tests pick their kernels by "chain_" and "tree_": neither may answer to them, argument types included
    assert not any("chain_" in n or "tree_" in n for n in mine), mine
    # ... and the unit brings no second copy of a chain kernel with the staging functions it takes from tpr_chain.hip.inc
    for name in ("chain_tool_wrench_kernel", "chain_tool_wrench_terms_kernel", "chain_tool_accel_kernel", "chain_tool_velocity_kernel"):
        assert sum(name in n for n in kernels) == 1, name


@pytest.mark.parametrize("key", sorted(AS_BUILT))
def test_state_in_registers(kernels, key):
    (r,) = [r for n, r in kernels.items() if key in n]
    in_registers(r, AS_BUILT[key], key)


def test_the_launch_s_lds_fits_the_cu():
    """Staging -- 3 arrays x 64 rows x (d | 1) doubles, or the outputs at pitch 7 where that is more -- plus forks x bank x 512
    bytes: at most 50 688 + 4 * 27 * 512 = 105 984 bytes (93 696 for the single evaluation), under the 160 KB of a CU; above 64 KB
    the launcher asks for the attribute."""
    args = open(os.path.join(ROOT, "toppra_amd", "csrc", "tpr_mount_args.hpp")).read()
    tree = open(os.path.join(ROOT, "toppra_amd", "csrc", "tpr_tree_args.hpp")).read()
    chain = open(os.path.join(ROOT, "toppra_amd", "csrc", "tpr_chain_args.hpp")).read()
    bank = (val("kMountBankSingle", args), val("kMountBankFused", args))
    forks, limit = val("kTreeMaxForks", tree), eval(re.search(r"kChainLdsBytes = ([0-9* ]+);", chain).group(1))
    assert bank == (21, 27) and forks == 4 and limit == 160 * 1024
    lds = lambda d, f, fused: max(3 * 64 * (d | 1), (3 if fused else 1) * 64 * 7) * 8 + f * bank[fused] * 64 * 8  # noqa: E731
    assert max(lds(d, f, 1) for d in range(1, 33) for f in range(forks + 1)) == lds(32, 4, 1) == 50688 + 4 * 27 * 512 == 105984 <= limit
    assert lds(32, 4, 0) == 50688 + 4 * 21 * 512 == 93696
    assert lds(32, 1, 1) <= 64 * 1024 < lds(32, 2, 1)  # (a chain never needs the attribute; two forks at 32 dof do)
    inc = open(os.path.join(ROOT, "toppra_amd", "csrc", "tpr_mount.hip.inc")).read()
    assert "mount_lds_bytes(kTreeMaxDof, kTreeMaxForks, true) == 105984" in inc and "<= (size_t)kChainLdsBytes" in inc
    unit = open(os.path.join(ROOT, "toppra_amd", "csrc", "tpr_mount_tu.hip")).read()
    assert unit.count("chain_allow_lds(") == 2 and "tpr::mount_lds_bytes(A->M.d, forks, true)" in unit and "tpr::mount_lds_bytes(A->M.d, forks, false)" in unit
    # the tree kernels' banks keep their own names and sizes
    assert val("kTreeBankSingle", tree) == 9 and val("kTreeBankFused", tree) == 18
