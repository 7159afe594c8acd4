"""The effective-mass accuracy table is the committed one: tests/effective_mass_cases.py's accuracy_table() -- the yardsticks the GPU
test's bounds are made from -- against the "cases" entry of profiles/effective_mass_accuracy.json, as
tests/test_rigid_accuracy_tables.py checks the siblings'.  (CPU only.)"""
import json
import os

import pytest

from tests import effective_mass_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_accuracy_table_is_the_committed_one():
    with open(os.path.join(ROOT, "profiles", "effective_mass_accuracy.json")) as fh:
        stored = json.load(fh)["cases"]
    table = ec.accuracy_table()
    assert sorted(stored) == sorted(table) == sorted(str(k) for k in ec.CASES)
    for key in ec.CASES:
        name = str(key)
        quantities = [ec.name_of(q, s) for q in ec.QUANTITIES for s in ec.sets_of(key)]
        assert sorted(stored[name]) == sorted(table[name]) == sorted(quantities), name
        for quantity, rec in table[name].items():
            # (to 1 %: a yardstick is a distance to an np.longdouble evaluation, whose sine and cosine are the host library's)
            assert stored[name][quantity]["yardstick"] == pytest.approx(rec["yardstick"], rel=1e-2), (name, quantity)
            assert stored[name][quantity]["bound"] == pytest.approx(ec.BOUND_FACTOR * stored[name][quantity]["yardstick"], rel=1e-12), (name, quantity)
            assert 0 < rec["yardstick"] < 1e-10
