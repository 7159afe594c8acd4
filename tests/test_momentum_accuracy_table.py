"""The accuracy table of the momentum tests is the committed one: tests/momentum_cases.py's accuracy_table() -- the yardsticks the
GPU tests' bounds are made from -- against the "cases" entry of profiles/momentum_accuracy.json, by the logic of
tests/test_rigid_accuracy_tables.py.  (CPU only.)"""
import json
import os

import pytest

from tests import momentum_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_accuracy_table_is_the_committed_one():
    with open(os.path.join(ROOT, "profiles", "momentum_accuracy.json")) as fh:
        stored = json.load(fh)["cases"]
    table = mc.accuracy_table()
    assert sorted(stored) == sorted(table) == sorted(str(k) for k in mc.CASES)
    for name in table:  # (to 1 %: a yardstick is the distance to an np.longdouble evaluation, whose sine and cosine are the host library's)
        assert sorted(stored[name]) == sorted(table[name]) == sorted(mc.name_of(q, s) for q in mc.QUANTITIES for s in mc.SETS), name
        for key, rec in table[name].items():
            assert stored[name][key]["yardstick"] == pytest.approx(rec["yardstick"], rel=1e-2), (name, key)
            assert stored[name][key]["bound"] == pytest.approx(mc.BOUND_FACTOR * stored[name][key]["yardstick"], rel=1e-12), (name, key)
