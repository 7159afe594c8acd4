"""The effective-mass kernel's resource usage, read from the built library's own code objects (tools/kernel_resources.py; no GPU,
no recompile): exactly one kernel answers to "effective_mass_kernel" and it answers to none of the names the chain, tree,
base-reaction, joint-load and momentum tests pick their kernels by; the articulated inertia, the velocities and a point's wrench
stay in registers at any dof: no scratch, no vector or scalar register spills (the walk's tables, the points and the output
pointers are read from the argument block where they are needed, a link's parameters are fetched in two parts, and the block's
place in the batch is worked out again for the outputs), no static LDS, at most the as-built register count plus 10 %; and the
launch's LDS arithmetic with the static_assert that proves it."""
import os
import re

import pytest

from tests.resource_support import built_kernels, in_registers, val

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toppra_amd", "csrc")

KEY = "effective_mass_kernel"
AS_BUILT = 116  # registers (vector + accumulator), read from the library as built


@pytest.fixture(scope="module")
def kernels():
    return built_kernels()


def test_exactly_one_effective_mass_kernel(kernels):
    import kernel_resources as kr  # (tools/ is on the path: tests/resource_support.py)
    mine = [n for n in kernels if KEY in n]
    assert len(mine) == 1 and "EffMassArgs" in mine[0], mine
    plain = kr.demangle(mine)[mine[0]]  # (the name itself where no demangler is installed)
    assert plain in (mine[0], "tpr::effective_mass_kernel(tpr::EffMassArgs)"), plain
    # the siblings' tests pick their kernels by these substrings of the names, argument types included
    for other in ("chain_", "tree_", "mount_wrench", "joint_wrench", "momentum_kernel"):
        assert other not in mine[0] and other not in plain, (other, mine)


def test_the_siblings_kernels_are_still_one_each(kernels):
    """The unit brings no second copy of a sibling's kernel with what it includes."""
    for name in ("momentum_kernel", "mount_wrench_kernel", "mount_wrench_terms_kernel",
                 "chain_tool_velocity_kernel", "chain_tool_accel_kernel", "chain_points_speed_kernel"):
        assert sum(name in n for n in kernels) == 1, name
    inc = open(os.path.join(CSRC, "tpr_effmass.hip.inc")).read() + open(os.path.join(CSRC, "tpr_effmass_tu.hip")).read()
    for sibling in ("tpr_chain.hip.inc", "tpr_tree.hip.inc", "tpr_mount.hip.inc", "tpr_joint.hip.inc", "tpr_momentum.hip.inc"):
        assert '#include "%s"' % sibling not in inc, sibling
    assert '#include "tpr_chain_rnea.hip.inc"' in inc and '#include "tpr_effmass_args.hpp"' in inc


def test_state_in_registers(kernels):
    (r,) = [r for n, r in kernels.items() if KEY in n]
    in_registers(r, AS_BUILT, KEY)


def test_the_launch_s_lds_fits_the_cu():
    """Slots of 512 bytes: 2 per link, 4 + 4 per point -- the second four lie over the staged rows, 2 (d | 1) slots, which are dead
    once the way up has read them -- and 21 per fork: at most (64 + 64 + 66 + 84) 512 = 142 336 bytes at 32 dof with 16 points and 4
    forks, under the 160 KB of a CU (with slots of their own the staged rows would make it 175 104: over).  Every robot and point
    set fits: the entry refuses none for its size.  Above 64 KB the launcher asks for the attribute."""
    args = open(os.path.join(CSRC, "tpr_effmass_args.hpp")).read()
    tree = open(os.path.join(CSRC, "tpr_tree_args.hpp")).read()
    chain = open(os.path.join(CSRC, "tpr_chain_args.hpp")).read()
    link, own, down, bank = (val(n, args) for n in ("kEffMassLink", "kEffMassOwn", "kEffMassDown", "kEffMassBank"))
    forks, points = val("kTreeMaxForks", tree), val("kChainMaxPoints", chain)
    limit = eval(re.search(r"kChainLdsBytes = ([0-9* ]+);", chain).group(1))
    assert (link, own, down, bank, forks, points, limit) == (2, 4, 4, 21, 4, 16, 160 * 1024)
    lds = lambda d, p, f: (link * d + own * p + max(down * p, 2 * (d | 1)) + bank * f) * 512  # noqa: E731
    every = [lds(d, p, f) for d in range(1, 33) for p in range(1, points + 1) for f in range(forks + 1)]
    assert max(every) == lds(32, 16, 4) == (64 + 64 + 66 + 84) * 512 == 142336 <= limit
    assert (64 + 64 + 64 + 66 + 84) * 512 == 175104 > limit
    assert lds(1, 1, 0) == 10 * 512 and lds(7, 4, 0) == (14 + 16 + 16) * 512 and lds(7, 1, 0) == (14 + 4 + 14) * 512
    assert lds(31, 1, 0) == 64 * 1024 < lds(32, 1, 0) and lds(1, 16, 0) > 64 * 1024  # (the attribute: 32 dof, or a full set)
    assert "effmass_lds_bytes(kTreeMaxDof, kChainMaxPoints, kTreeMaxForks) == 142336" in args and "<= (size_t)kChainLdsBytes" in args
    assert "constexpr size_t effmass_lds_bytes(int d, int points, int forks)" in args and "static_assert(" in args
    unit = open(os.path.join(CSRC, "tpr_effmass_tu.hip")).read()
    assert unit.count("chain_allow_lds(") == 1 and "tpr::effmass_lds_bytes(A->M.d, A->P.count, forks)" in unit
    kernel = open(os.path.join(CSRC, "tpr_effmass.hip.inc")).read()
    assert "effmass_shared_slots(d, count)" in kernel and "extern __shared__ double effmass_lds[];" in kernel and "static __shared__" not in kernel


def test_the_unit_is_built_and_checked():
    from toppra_amd import build
    assert "tpr_effmass_tu.hip" in build.SOURCES and ("effmass", "tpr_effmass_tu.hip", []) in build.compile_jobs()
    text = open(os.path.join(ROOT, "toppra_amd", "build.py")).read()
    assert re.search(r'name\.startswith\(\([^)]*"effmass"', text)
