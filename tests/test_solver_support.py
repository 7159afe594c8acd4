"""tests/solver_support.py on the CPU: the comparison every GPU parity test of the solver leans on must itself fail when it should,
and say where; the flag mapping and the tracer's name matcher on hand-written inputs.  No GPU, no tracer, no child process."""
import numpy as np
import pytest

from tests.solver_support import dispatches, oracle_flags, same, same_array

KINDS = np.array(["plain", "vinf", "ahuge", "plain", "still"])


def result():
    K = np.arange(30, dtype=np.float64).reshape(5, 3, 2)
    K[1], K[4, 2, 1] = np.nan, np.nan
    return {"status": np.array([0, 1, 0, 0, 0]), "K": K, "sd2": np.linspace(0, 1, 15).reshape(5, 3)}


def failure(got, want, keys=("K", "sd2"), kinds=None):
    """The arguments of the AssertionError that `same` must raise, as text."""
    with pytest.raises(AssertionError) as err:
        same(got, want, keys, ("the case", 7), kinds)
    return repr(err.value.args)


def test_identical_results_with_nans_in_matching_places_pass():
    same(result(), result(), ("K", "sd2"), ("identical",))
    same(result(), result(), ("K", "sd2"), ("identical",), KINDS)


def test_a_status_mismatch_fails_and_names_the_trajectory():
    got = result()
    got["status"][3] = 1
    text = failure(got, result())
    assert "the case" in text and "'status'" in text and "[3]" in text
    assert "'plain'" in failure(got, result(), kinds=KINDS)


def test_a_value_mismatch_fails_and_names_key_trajectory_and_kind():
    got = result()
    got["K"][2, 1, 0] = np.nextafter(got["K"][2, 1, 0], np.inf)  # one bit
    text = failure(got, result())
    assert "the case" in text and "'K'" in text and "[2]" in text and "'sd2'" not in text
    text = failure(got, result(), kinds=KINDS)
    assert "'ahuge'" in text and "'plain'" not in text
    got["sd2"][0, 0] = 0.5
    got["K"][4, 0, 0] = -1.0
    assert "[2, 4]" in failure(got, result()) and "[0]" in failure(got, result(), keys=("sd2",))


def test_a_nan_on_one_side_only_fails():
    got = result()
    got["K"][1, 0, 0] = 3.0  # a number where the other side has NaN ...
    assert "'K'" in failure(got, result()) and "[1]" in failure(got, result())
    got = result()
    got["sd2"][3, 2] = np.nan  # ... and NaN where it has a number
    text = failure(got, result(), kinds=KINDS)
    assert "'sd2'" in text and "[3]" in text and "'plain'" in text


def test_a_shape_mismatch_fails():
    got = result()
    got["sd2"] = got["sd2"][:, :2]
    text = failure(got, result())
    assert "'sd2'" in text and "(5, 2)" in text and "(5, 3)" in text
    with pytest.raises(AssertionError):
        same_array(np.zeros(()), np.zeros(1), "a scalar is not a vector of one")


def test_status_is_compared_only_where_the_authority_has_one():
    want = result()
    del want["status"]
    got = result()
    got["status"][:] = 5
    same(got, want, ("K", "sd2"), ("no status in want",))
    same({"K": got["K"]}, want, ("K",), ("no status at all",))
    with pytest.raises(KeyError):
        same({"K": got["K"]}, result(), ("K",), ("want has a status, got has none",))
    got = result()
    got["status"][0] = 1
    assert "'status'" in failure(got, result(), keys=("K", "sd2", "status"))  # ("status" among the keys is the same exact comparison)


def test_same_array_on_bare_arrays():
    x = result()["K"]
    same_array(x, x.copy(), ("X",))
    same_array(x[0], x[0].copy(), "one trajectory")
    same_array(3.0, 3.0, "scalars")
    y = x.copy()
    y[3, 0, 1] += 1.0
    with pytest.raises(AssertionError) as err:
        same_array(y, x, ("X", "dense"), KINDS)
    text = repr(err.value.args)
    assert "'dense'" in text and "[3]" in text and "'plain'" in text
    with pytest.raises(AssertionError):
        same_array(np.array([np.nan]), np.array([0.0]), "NaN against a number")


def test_oracle_flags_is_the_mapping_written_out_by_hand():
    from oracle import oracle
    for vel in (False, True):
        for interp in (False, True):
            for acc in (False, True):
                by_hand = (oracle.FLAG_VEL if vel else 0) + (oracle.FLAG_ACC if acc else 0) + (oracle.FLAG_INTERP if interp else 0)
                assert oracle_flags(oracle, vel, interp, acc) == by_hand, (vel, interp, acc)
            assert oracle_flags(oracle, vel, interp) == oracle_flags(oracle, vel, interp, True)
    assert len({oracle.FLAG_VEL, oracle.FLAG_ACC, oracle.FLAG_INTERP, 0}) == 4 and not oracle.FLAG_VEL & oracle.FLAG_ACC
    assert oracle_flags(oracle, True, True) == oracle.DEFAULT_FLAGS
    assert oracle_flags(oracle, True, False) == oracle.DEFAULT_FLAGS & ~oracle.FLAG_INTERP
    assert oracle_flags(oracle, False, True) == oracle.FLAG_ACC | oracle.FLAG_INTERP


def test_dispatches_counts_by_name_and_by_first_template_argument():
    calls = [("void tpr::cert_solve_kernel<7, false, true>(tpr::GroupArgs)", 3),
             ("_ZN3tpr17cert_solve_kernelILi7ELb1ELb0EEEvNS_9GroupArgsE", 2),
             ("void tpr::cert_solve_kernel<17, false, true>(tpr::GroupArgs)", 50),
             ("_ZN3tpr17cert_solve_kernelILi17ELb1ELb0EEEvNS_9GroupArgsE", 70),
             ("void tpr::cert_solve_kernel<9, false, true>(tpr::GroupArgs)", 11),
             ("void tpr::group_solve_kernel<7, 8>(tpr::GroupArgs)", 5),
             ("void tpr::cert_feasible_kernel<7, true>(tpr::GroupArgs)", 1),
             ("tpr::pair_solve_kernel(tpr::GroupArgs)", 4)]
    assert dispatches(calls, "cert_solve_kernel", 7) == 5
    assert dispatches(calls, "cert_solve_kernel", 17) == 120
    assert dispatches(calls, "cert_solve_kernel", 9) == 11
    assert dispatches(calls, "cert_solve_kernel", 1) == 0
    assert dispatches(calls, "cert_solve_kernel") == 136
    assert dispatches(calls, "group_solve_kernel", 7) == 5 and dispatches(calls, "cert_feasible_kernel", 7) == 1
    assert dispatches(calls, "pair_solve_kernel") == 4 and dispatches(calls, "pair_solve_kernel", 7) == 0
    assert dispatches(calls, "wave_solve_kernel") == 0 and dispatches([], "cert_solve_kernel", 7) == 0
