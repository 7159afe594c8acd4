"""The tree kernels' resource usage, read from the built library's own code objects (tools/kernel_resources.py; no GPU, no
recompile), as tests/test_chain_resources.py reads the chain kernels': exactly three kernels, no scratch, no static LDS, registers
under the committed ceilings (as built plus 10 %), and the launcher's LDS arithmetic.

As built: the single evaluation takes the chain kernel's 95 registers, the fused kernel 129 against the chain's 121 (the three
levels of a fork's state on their way to and from the bank), the one-after-the-other kernel 143 against 135.  No kernel spills a
vector register; the compiler parks 3 / 3 / 5 scalar registers in lanes of a vector register across the loops (the chain's
runtime-dof kernels park 8), which costs no memory traffic."""
import os
import re

import pytest

from tests.resource_support import built_kernels, in_registers, val

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# as built: registers (vector + accumulator)
TREE = {"tree_inverse_dynamics_kernel": 95, "tree_torque_terms_kernelILb1E": 129, "tree_torque_terms_kernelILb0E": 143}


@pytest.fixture(scope="module")
def kernels():
    return built_kernels()


def test_exactly_three_tree_kernels(kernels):
    tree = sorted(n for n in kernels if "tree_" in n)
    assert len(tree) == 3, tree
    for key in TREE:
        assert sum(key in n for n in tree) == 1, (key, tree)
    # the chain tests pick their kernels by "chain_": no tree kernel may answer to it, and the tree unit brings no second copy of one
    assert not any("chain_" in n for n in tree)


def test_no_scratch_no_static_lds_and_registers_under_the_ceiling(kernels):
    for key, regs in TREE.items():
        (r,) = [r for n, r in kernels.items() if key in n]
        in_registers(r, regs, key, parked_scalars=True)  # (their LDS is dynamic: at most 160 KB, checked at launch)


def _constants():
    text = open(os.path.join(ROOT, "toppra_amd", "csrc", "tpr_tree_args.hpp")).read()
    chain = open(os.path.join(ROOT, "toppra_amd", "csrc", "tpr_chain_args.hpp")).read()
    return {"slots": (val("kChainSlotsSingle", chain), val("kChainSlotsFused", chain)), "bank": (val("kTreeBankSingle", text), val("kTreeBankFused", text)),
            "forks": val("kTreeMaxForks", text), "lds": eval(re.search(r"kChainLdsBytes = ([0-9* ]+);", chain).group(1))}


def test_the_launch_s_lds_fits_the_cu():
    """d * slots * 512 + forks * bank * 512 bytes: the single state fits 160 KB at 32 dof with 4 forks (149 504 bytes); with one
    fork the fused state fits up to 17 dof and the launcher runs the evaluations one after another from 18 on."""
    c = _constants()
    assert c["slots"] == (8, 17) and c["bank"] == (9, 18) and c["forks"] == 4 and c["lds"] == 160 * 1024
    lds = lambda d, forks, fused: (d * c["slots"][fused] + forks * c["bank"][fused]) * 64 * 8  # noqa: E731
    assert lds(32, 4, 0) == 32 * 8 * 512 + 4 * 9 * 512 == 149504 <= c["lds"]
    assert lds(17, 1, 1) <= c["lds"] < lds(18, 1, 1)
    assert lds(18, 0, 1) <= c["lds"] < lds(19, 0, 1)  # (a chain-shaped tree switches where the chain kernels do)
    header = open(os.path.join(ROOT, "include", "toppra_hip.h")).read()
    assert re.search(r"#define TPR_TREE_MAX_FORKS (\d+)", header).group(1) == "4"
