"""The accuracy tables of the rigid-body family are the committed ones: every cases module's accuracy_table() -- the yardsticks
the GPU tests' bounds are made from -- against the "cases" entry of its profile.  (CPU only.)"""
import importlib
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = {"chain_cases": "chain_dynamics_accuracy.json", "tree_cases": "tree_dynamics_accuracy.json",
            "tool_accel_cases": "tool_accel_accuracy.json", "tool_wrench_cases": "tool_wrench_accuracy.json",
            "control_points_cases": "control_points_accuracy.json", "base_wrench_cases": "base_wrench_accuracy.json",
            "joint_load_cases": "joint_load_accuracy.json", "momentum_cases": "momentum_accuracy.json"}
# (optional, per family: the keys the table must have -- its cases, and the quantities of every case)
KEYS = {"momentum_cases": lambda mc: ([str(k) for k in mc.CASES], [mc.name_of(q, s) for q in mc.QUANTITIES for s in mc.SETS])}


@pytest.mark.parametrize("module", sorted(FAMILIES))
def test_accuracy_table_is_the_committed_one(module):
    cases = importlib.import_module("tests." + module)
    with open(os.path.join(ROOT, "profiles", FAMILIES[module])) as fh:
        stored = json.load(fh)["cases"]
    table = cases.accuracy_table()
    case_keys, quantity_keys = KEYS[module](cases) if module in KEYS else (table, None)
    assert sorted(stored) == sorted(table) == sorted(case_keys)
    for name in table:  # (to 1 %: a yardstick is the distance to an np.longdouble evaluation, whose sine and cosine are the host library's)
        assert sorted(stored[name]) == sorted(table[name]) == sorted(quantity_keys or table[name]), name
        for key, rec in table[name].items():
            assert stored[name][key]["yardstick"] == pytest.approx(rec["yardstick"], rel=1e-2), (name, key)
            assert stored[name][key]["bound"] == pytest.approx(cases.BOUND_FACTOR * stored[name][key]["yardstick"], rel=1e-12), (name, key)
            if "restatement" in rec:  # (joint loads: the link-local restatement's share of the bound)
                assert stored[name][key]["restatement"] == pytest.approx(rec["restatement"], rel=1e-2), (name, key)
