"""The momentum kernel's resource usage, read from the built library's own code objects (tools/kernel_resources.py; no GPU, no
recompile): exactly one kernel answers to "momentum_kernel" and it answers to none of the names the chain, tree, base-reaction and
joint-load tests pick their kernels by; a point's whole state -- W, p, v, w and the running P, L, T2 -- stays in registers at any
dof: no scratch, no vector or scalar register spills (the walk's byte tables, the mount's frame and the output pointers are read
from the argument block where they are needed, and a link's parameters are fetched in two parts), no static LDS (the dynamic LDS
stages a block's inputs and outputs and keeps the forks' banks), at most the as-built register count plus 10 %, and the launch's
LDS arithmetic."""
import os
import re

import pytest

from tests.resource_support import built_kernels, in_registers, val

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEY = "momentum_kernel"
AS_BUILT = 116  # registers (vector + accumulator), read from the library as built


@pytest.fixture(scope="module")
def kernels():
    return built_kernels()


def test_exactly_one_momentum_kernel(kernels):
    import kernel_resources as kr  # (tools/ is on the path: tests/resource_support.py)
    mine = [n for n in kernels if KEY in n]
    assert len(mine) == 1 and "MomentumArgs" in mine[0], mine
    plain = kr.demangle(mine)[mine[0]]  # (the name itself where no demangler is installed)
    assert plain in (mine[0], "tpr::momentum_kernel(tpr::MomentumArgs)"), plain
    # the siblings' tests pick their kernels by these substrings of the names, argument types included
    for other in ("chain_", "tree_", "mount_wrench", "joint_wrench"):
        assert other not in mine[0] and other not in plain, (other, mine)
    # ... and the unit brings no second copy of a sibling's kernel with what it includes
    for name in ("mount_wrench_kernel", "mount_wrench_terms_kernel", "chain_tool_velocity_kernel", "chain_tool_accel_kernel",
                 "chain_points_speed_kernel"):
        assert sum(name in n for n in kernels) == 1, name


def test_state_in_registers(kernels):
    (r,) = [r for n, r in kernels.items() if KEY in n]
    in_registers(r, AS_BUILT, KEY)


def test_the_launch_s_lds_fits_the_cu():
    """Staging -- 2 arrays x 64 rows x (d | 1) doubles, or the 64 output rows of 9 doubles where that is more -- plus forks x 18 x
    512 bytes: at most 33 792 + 4 * 18 * 512 = 70 656 bytes, under the 160 KB of a CU; above 64 KB the launcher asks for the
    attribute -- only the widest tree does."""
    csrc = os.path.join(ROOT, "toppra_amd", "csrc")
    args = open(os.path.join(csrc, "tpr_momentum_args.hpp")).read()
    tree = open(os.path.join(csrc, "tpr_tree_args.hpp")).read()
    chain = open(os.path.join(csrc, "tpr_chain_args.hpp")).read()
    bank, out = val("kMomentumBank", args), val("kMomentumOut", args)
    forks, limit = val("kTreeMaxForks", tree), eval(re.search(r"kChainLdsBytes = ([0-9* ]+);", chain).group(1))
    assert bank == 18 and out == 9 and out % 2 == 1 and forks == 4 and limit == 160 * 1024
    lds = lambda d, f: max(2 * 64 * (d | 1), 64 * out) * 8 + f * bank * 64 * 8  # noqa: E731
    assert max(lds(d, f) for d in range(1, 33) for f in range(forks + 1)) == lds(32, 4) == 33792 + 4 * 18 * 512 == 70656 <= limit
    assert lds(1, 0) == lds(3, 0) == 64 * 9 * 8 < lds(4, 0) == 2 * 64 * 5 * 8  # (below 4 dof the outputs size the staging area)
    assert lds(32, 3) <= 64 * 1024 < lds(32, 4) and lds(27, 4) <= 64 * 1024 < lds(28, 4)
    assert "momentum_lds_bytes(kTreeMaxDof, kTreeMaxForks) == 70656" in args and "<= (size_t)kChainLdsBytes" in args
    assert "constexpr size_t momentum_lds_bytes(" in args
    unit = open(os.path.join(csrc, "tpr_momentum_tu.hip")).read()
    assert unit.count("chain_allow_lds(") == 1 and "tpr::momentum_lds_bytes(A->M.d, forks)" in unit
    # the unit takes none of its siblings' kernels with what it includes
    inc = open(os.path.join(csrc, "tpr_momentum.hip.inc")).read()
    assert '#include "tpr_mount.hip.inc"' not in inc and '#include "tpr_chain.hip.inc"' not in inc
    # the siblings' banks keep their own names and sizes
    mount = open(os.path.join(csrc, "tpr_mount_args.hpp")).read()
    assert val("kMountBankSingle", mount) == 21 and val("kMountBankFused", mount) == 27
