"""The joint-wrench kernels' resource usage, read from the built library's own code objects (tools/kernel_resources.py; no GPU,
no recompile): exactly three kernels answer to "joint_wrench" and none of them to the names the chain and tree tests pick their
kernels by; no scratch, no vector register spills, no static LDS (the dynamic LDS is the tree kernels': the per-link state and the
forks' banks; the outputs leave by direct stores), at most the as-built register count plus 10 %, and the launch's LDS arithmetic
against the struct sizes."""
import ctypes
import os
import re

import pytest

from tests.resource_support import built_kernels, in_registers, val

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# as built: registers (vector + accumulator)
AS_BUILT = {"joint_wrench_kernelE": 91, "joint_wrench_terms_kernelILb1E": 121, "joint_wrench_terms_kernelILb0E": 143}


@pytest.fixture(scope="module")
def kernels():
    return built_kernels()


def test_exactly_three_joint_kernels(kernels):
    mine = sorted(n for n in kernels if "joint_wrench" in n)
    assert len(mine) == 3, mine
    for key in AS_BUILT:
        assert sum(key in n for n in mine) == 1, (key, mine)
    # the chain and tree tests pick their kernels by "chain_" and "tree_": neither may answer to them, argument types included
    assert not any("chain_" in n or "tree_" in n for n in mine), mine
    # ... and the unit brings no second copy of a tree kernel with the banks it takes from tpr_tree_walk.hip.inc
    for name in ("tree_inverse_dynamics_kernel", "tree_torque_terms_kernelILb1E", "tree_torque_terms_kernelILb0E"):
        assert sum(name in n for n in kernels) == 1, name


@pytest.mark.parametrize("key", sorted(AS_BUILT))
def test_no_scratch_no_static_lds_and_registers_under_the_ceiling(kernels, key):
    (r,) = [r for n, r in kernels.items() if key in n]
    in_registers(r, AS_BUILT[key], key, parked_scalars=True)


def test_the_launch_s_lds_fits_the_cu():
    """d * slots * 512 + forks * bank * 512 bytes, the tree kernels': the single state serves 32 dof with 4 forks within 160 KB
    (149 504 bytes: the sequential mode), the fused state a chain to 18 dof and one fork to 17; the outputs take no LDS."""
    tree = open(os.path.join(ROOT, "toppra_amd", "csrc", "tpr_tree_args.hpp")).read()
    chain = open(os.path.join(ROOT, "toppra_amd", "csrc", "tpr_chain_args.hpp")).read()
    args = open(os.path.join(ROOT, "toppra_amd", "csrc", "tpr_joint_args.hpp")).read()
    slots = (val("kChainSlotsSingle", chain), val("kChainSlotsFused", chain))
    bank = (val("kTreeBankSingle", tree), val("kTreeBankFused", tree))
    forks, limit = val("kTreeMaxForks", tree), eval(re.search(r"kChainLdsBytes = ([0-9* ]+);", chain).group(1))
    assert slots == (8, 17) and bank == (9, 18) and forks == 4 and limit == 160 * 1024
    lds = lambda d, f, fused: (d * slots[fused] + f * bank[fused]) * 64 * 8  # noqa: E731
    assert max(lds(d, f, 0) for d in range(1, 33) for f in range(forks + 1)) == lds(32, 4, 0) == 149504 <= limit
    assert lds(18, 0, 1) <= limit < lds(19, 0, 1) and lds(17, 1, 1) <= limit < lds(18, 1, 1)
    assert lds(15, 1, 1) == (15 * 17 + 18) * 512  # (the torso: fused)
    assert "constexpr size_t joint_lds_bytes(int d, int forks, bool fused) { return tree_lds_bytes(d, forks, fused); }" in args
    assert "joint_lds_bytes(kTreeMaxDof, kTreeMaxForks, false) <= (size_t)kChainLdsBytes" in args
    assert "joint_terms_fused(17, 1) && !joint_terms_fused(18, 1)" in args and "joint_terms_fused(18, 0) && !joint_terms_fused(19, 0)" in args
    unit = open(os.path.join(ROOT, "toppra_amd", "csrc", "tpr_joint_tu.hip")).read()
    assert unit.count("chain_allow_lds(") == 3 and unit.count("tpr::joint_lds_bytes(A->M.d, forks, false)") == 2
    assert "tpr::joint_lds_bytes(A->M.d, forks, true)" in unit and "tpr::joint_terms_fused(A->M.d, forks)" in unit


def test_the_sections_struct_is_the_header_s():
    from toppra_amd import _capi
    header = open(os.path.join(ROOT, "include", "toppra_hip.h")).read()
    assert re.search(r"#define TPR_JOINT_MAX_SECTIONS (\d+)", header).group(1) == "8" and _capi.JOINT_MAX_SECTIONS == 8
    args = open(os.path.join(ROOT, "toppra_amd", "csrc", "tpr_joint_args.hpp")).read()
    assert re.search(r"kJointMaxSections = (\d+);", args).group(1) == "8"
    # the C struct: a count, 8 links, a word of padding, 8 x (9 + 3) doubles; the kernels' copy adds the mask and the lowest link
    assert ctypes.sizeof(_capi.tpr_joint_sections) == 4 + 4 * 8 + 4 + 8 * 12 * 8 == 808
    assert _capi.tpr_joint_sections.rot.offset == 40 and _capi.tpr_joint_sections.origin.offset == 40 + 8 * 9 * 8
    assert "sizeof(JointSections) == 12 + 4 * kJointMaxSections + 4 + 8 * 12 * kJointMaxSections" in args
