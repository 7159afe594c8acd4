"""Which refusal wins when two arguments of a dense-row entry are bad at once.  The fifteen entries of include/toppra_hip.h that
run the dense-row passes -- solve, TOPPRAsd, controllable / feasible / reachable sets, each fed from arrays
(``tpr_*_dense_batch``), from path samples (``tpr_*_sampled_batch``) and from samples plus stage boxes
(``tpr_*_sampled_boxed_batch``) -- through ctypes, with buffers 64 doubles long.  Every call but the ones with B = 0 is refused,
and those launch nothing.  The order is behaviour:

* dense: tpr_init, the problem pointer, B / N, nC (unsupported), the six arrays;
* sampled: tpr_init, the problem pointer, B / N, d (unsupported), grid / qs / qss, vlim under its flag, alim under its flag, the
  row count (unsupported);
* boxed: what the sampled entries check, then vlim (unsupported), then low / high;
* then the pass's own pointers.

The shapes are the smallest whose size products are all non-zero: B = 1, N = 1, nC = 2 (dense), d = 1 (sampled, boxed).  Two
parts need no GPU: what an entry answers before tpr_init has succeeded, and the Python signatures of the fifteen ``batch.*``
functions (parameter order and defaults are API, and they differ between siblings)."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, HIP, UNSUPPORTED = 0, -1, -2, -3
HAS_VELOCITY, HAS_ACCELERATION, ACC_INTERPOLATION = 1, 2, 4

FAMILIES = ("dense", "sampled", "sampled_boxed")
# pass: (the entry's own pointers, in argument order; which of them it requires; its refusal of a missing one)
PASSES = {
    "solve": (("r",), ("r", "K"), None),
    "solve_desired_duration": (("desired", "atol", "r", "alpha"), ("r", "K", "desired"), b"result.K and desired are required"),
    "controllable_sets": (("sdmin", "sdmax", "K"), ("sdmin", "sdmax", "K"), b"sdmin/sdmax/K are required"),
    "feasible_sets": (("X",), ("X",), b"X is required"),
    "reachable_sets": (("sdmin", "sdmax", "L", "X"), ("sdmin", "sdmax", "L"), b"sdmin/sdmax/L are required"),
}
SOLVE_PREFIX = {"dense": b"dense solve", "sampled": b"sampled solve", "sampled_boxed": b"boxed sampled solve"}
ENTRIES = [(family, name) for family in FAMILIES for name in PASSES]
IDS = ["tpr_%s_%s_batch" % (name, family) for family, name in ENTRIES]
SAMPLED_ENTRIES = [e for e in ENTRIES if e[0] != "dense"]
SAMPLED_IDS = [i for e, i in zip(ENTRIES, IDS) if e[0] != "dense"]
BOXED_ENTRIES = [e for e in ENTRIES if e[0] == "sampled_boxed"]
BOXED_IDS = [i for e, i in zip(ENTRIES, IDS) if e[0] == "sampled_boxed"]
DENSE_ENTRIES = [e for e in ENTRIES if e[0] == "dense"]
DENSE_IDS = [i for e, i in zip(ENTRIES, IDS) if e[0] == "dense"]

NULL_PROBLEM = {"dense": b"null dense problem", "sampled": b"null sampled problem", "sampled_boxed": b"null sampled problem"}
BN = {"dense": b"dense problem: B >= 0, N >= 1", "sampled": b"sampled problem: B >= 0, N >= 1",
      "sampled_boxed": b"sampled problem: B >= 0, N >= 1"}
DENSE_NC = b"dense problem: 2 <= nC <= 122 rows per stage (incl. the two x_next rows)"
DENSE_ARRAYS = b"dense problem: a, b, c, low, high, deltas are required"
SAMPLED_DOF = b"sampled problem: dof must be in [1, TPR_MAX_DOF]"
SAMPLED_ARRAYS = b"sampled problem: grid, qs, qss are required"
NO_VLIM = b"TPR_HAS_VELOCITY without vlim"
NO_ALIM = b"TPR_HAS_ACCELERATION without alim"
SAMPLED_ROWS = b"sampled problem: more than 122 rows per stage (2 + 4 d under Interpolation: d <= 30; Collocation: d <= 32)"
BOXED_VLIM = (b"boxed sampled problem: vlim must be NULL and TPR_HAS_VELOCITY clear (the boxes carry every first-order constraint: "
              b"make the limits a source of tpr_stage_boxes_batch)")
BOXED_ARRAYS = b"boxed sampled problem: low, high are required"

_BUF = np.zeros(64)
_STATUS = np.zeros(64, dtype=np.int32)


def own_refusal(family, name):
    """The exact message of ``name``'s refusal of a missing pointer of its own."""
    return PASSES[name][2] or SOLVE_PREFIX[family] + b": r->K is required"


def problem(family, **fields):
    """A valid problem of ``family`` at the smallest shape on the shared buffer, ``fields`` in place of its own; a field given as
    None is a null pointer."""
    from toppra_amd import _capi
    p = _BUF.ctypes.data
    if family == "dense":
        values = dict(B=1, N=1, nC=2, flags=0, a=p, b=p, c=p, low=p, high=p, deltas=p)
        values.update(fields)
        return _capi.tpr_dense_problem(**values)
    values = dict(B=1, d=1, N=1, flags=0, grid=p, qs=p, qss=p)
    values.update(fields)
    return _capi.tpr_sampled_problem(**values)


def call(family, name, prob, null=(), low=True, high=True):
    """(code, message) of one call of tpr_<name>_<family>_batch: ``prob`` may be None (NULL); ``null`` names the pointers of the
    pass handed over as NULL ("r": the result struct, "K" of solve / TOPPRAsd: its K field); ``low`` / ``high`` False: NULL
    boxes."""
    from toppra_amd import _capi
    lib = _capi.load()
    p = _BUF.ctypes.data
    result = _capi.tpr_result(sd2=p, sd=p, u=p, K=None if "K" in null else p, status=_STATUS.ctypes.data)
    args = [None if prob is None else ctypes.byref(prob)]
    if family == "sampled_boxed":
        args += [p if low else None, p if high else None]
    for arg in PASSES[name][0]:
        if arg == "atol":
            args.append(1e-5)
        elif arg == "r":
            args.append(None if "r" in null else ctypes.byref(result))
        else:
            args.append(None if arg in null else p)
    rc = getattr(lib, "tpr_%s_%s_batch" % (name, family))(*args, None)
    return rc, lib.tpr_last_error()


def refused(got, code, message):
    """The code and the whole message, nothing before or after it."""
    rc, msg = got
    assert rc == code and msg == message, (rc, msg)


# ---- without a GPU ----------------------------------------------------------------------------------------------------------

def test_every_entry_asks_for_tpr_init_first():
    """In a process that never called tpr_init: a null problem and null outputs are answered with TPR_E_HIP."""
    code = (
        "import sys\n"
        "sys.path.insert(0, %r)\n"
        "from tests import test_dense_refusal_order as t\n"
        "for family, name in t.ENTRIES:\n"
        "    rc, msg = t.call(family, name, None, null=t.PASSES[name][1], low=False, high=False)\n"
        "    assert rc == t.HIP and msg == b'tpr_init() has not succeeded', (family, name, rc, msg)\n"
        "print('entries', len(t.ENTRIES))\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, TOPPRA_HIP_NO_TORCH="1"))
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "entries 15", out.stdout


SIGNATURES = {
    "solve_dense_batch": "(a, b, c, low, high, deltas, sd_start=None, sd_end=None, want_sd=False, squared=False, active=None)",
    "solve_desired_duration_dense_batch": "(a, b, c, low, high, deltas, desired_duration, sd_start=None, sd_end=None, atol=1e-05, active=None, squared=False)",
    "controllable_sets_dense_batch": "(a, b, c, low, high, deltas, sdmin, sdmax, squared=False, active=None)",
    "feasible_sets_dense_batch": "(a, b, c, low, high, deltas, active=None)",
    "reachable_sets_dense_batch": "(a, b, c, low, high, deltas, sdmin, sdmax, want_X=False, active=None, squared=False)",
    "solve_sampled_batch": "(grid, qs, qss, vlim, alim, sd_start=None, sd_end=None, interpolation=True, want_sd=False, squared=False, active=None)",
    "solve_desired_duration_sampled_batch": "(grid, qs, qss, vlim, alim, desired_duration, sd_start=None, sd_end=None, atol=1e-05, interpolation=True, active=None, squared=False)",
    "controllable_sets_sampled_batch": "(grid, qs, qss, vlim, alim, sdmin, sdmax, interpolation=True, squared=False, active=None)",
    "feasible_sets_sampled_batch": "(grid, qs, qss, vlim, alim, interpolation=True, active=None)",
    "reachable_sets_sampled_batch": "(grid, qs, qss, vlim, alim, sdmin, sdmax, interpolation=True, want_X=False, active=None, squared=False)",
    "solve_sampled_boxed_batch": "(grid, qs, qss, alim, low, high, sd_start=None, sd_end=None, interpolation=True, want_sd=False, squared=False, active=None, vlim=None)",
    "solve_desired_duration_sampled_boxed_batch": "(grid, qs, qss, alim, low, high, desired_duration, sd_start=None, sd_end=None, atol=1e-05, interpolation=True, active=None, squared=False, vlim=None)",
    "controllable_sets_sampled_boxed_batch": "(grid, qs, qss, alim, low, high, sdmin, sdmax, interpolation=True, squared=False, active=None, vlim=None)",
    "feasible_sets_sampled_boxed_batch": "(grid, qs, qss, alim, low, high, interpolation=True, active=None, vlim=None)",
    "reachable_sets_sampled_boxed_batch": "(grid, qs, qss, alim, low, high, sdmin, sdmax, interpolation=True, want_X=False, active=None, squared=False, vlim=None)",
}


def test_python_signatures_are_the_recorded_ones():
    from toppra_amd import batch
    assert sorted(SIGNATURES) == sorted("%s_%s_batch" % (name, family) for family, name in ENTRIES)
    assert {n: str(inspect.signature(getattr(batch, n))) for n in SIGNATURES} == SIGNATURES
    assert all(getattr(batch, n).__doc__ for n in SIGNATURES)


# ---- with a GPU: every call is refused, or has B = 0 -------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("family, name", ENTRIES, ids=IDS)
def test_a_bad_problem_wins_over_null_outputs(gpu, family, name):
    null = PASSES[name][1]
    refused(call(family, name, None, null=null, low=False, high=False), BADARG, NULL_PROBLEM[family])
    # B / N before what follows them: a row count / dof out of range as well
    extra = {"nC": 1} if family == "dense" else {"d": 0}
    refused(call(family, name, problem(family, B=-1, **extra), null=null), BADARG, BN[family])
    refused(call(family, name, problem(family, N=0, **extra), null=null), BADARG, BN[family])


@pytest.mark.gpu
@pytest.mark.parametrize("family, name", DENSE_ENTRIES, ids=DENSE_IDS)
def test_dense_entries_refuse_in_their_order(gpu, family, name):
    null = PASSES[name][1]
    # the row count before the arrays
    for nC in (1, 123):
        refused(call(family, name, problem(family, nC=nC, a=None), null=null), UNSUPPORTED, DENSE_NC)
    # each array before the pass's own pointers
    for field in ("a", "b", "c", "low", "high", "deltas"):
        refused(call(family, name, problem(family, **{field: None}), null=null), BADARG, DENSE_ARRAYS)


@pytest.mark.gpu
@pytest.mark.parametrize("family, name", SAMPLED_ENTRIES, ids=SAMPLED_IDS)
def test_sampled_and_boxed_entries_refuse_in_their_order(gpu, family, name):
    null = PASSES[name][1]
    p = _BUF.ctypes.data
    both = HAS_VELOCITY | HAS_ACCELERATION | ACC_INTERPOLATION
    # the dof before the samples
    for d in (0, 33):
        refused(call(family, name, problem(family, d=d, grid=None), null=null), UNSUPPORTED, SAMPLED_DOF)
    # the samples before the limits
    for field in ("grid", "qs", "qss"):
        refused(call(family, name, problem(family, flags=both, **{field: None}), null=null), BADARG, SAMPLED_ARRAYS)
    # vlim before alim, alim before the row count (31 dof under Interpolation: 126 rows)
    refused(call(family, name, problem(family, flags=both), null=null), BADARG, NO_VLIM)
    refused(call(family, name, problem(family, d=31, flags=both, vlim=p), null=null), BADARG, NO_ALIM)
    # the row count before the boxes and the pass's own pointers
    rows = problem(family, d=31, flags=both, vlim=p, alim=p)
    refused(call(family, name, rows, null=null, low=False, high=False), UNSUPPORTED, SAMPLED_ROWS)
    # 30 dof fit: the next refusal is the boxed entries' vlim, else the pass's own
    fits = problem(family, d=30, flags=both, vlim=p, alim=p)
    want = (UNSUPPORTED, BOXED_VLIM) if family == "sampled_boxed" else (BADARG, own_refusal(family, name))
    refused(call(family, name, fits, null=null, low=False, high=False), *want)


@pytest.mark.gpu
@pytest.mark.parametrize("family, name", BOXED_ENTRIES, ids=BOXED_IDS)
def test_boxed_entries_refuse_vlim_then_the_boxes(gpu, family, name):
    null = PASSES[name][1]
    p = _BUF.ctypes.data
    # vlim set and low null: vlim -- with and without its flag
    refused(call(family, name, problem(family, vlim=p), null=null, low=False), UNSUPPORTED, BOXED_VLIM)
    refused(call(family, name, problem(family, vlim=p, flags=HAS_VELOCITY), null=null, low=False, high=False), UNSUPPORTED, BOXED_VLIM)
    # the flag without vlim is the sampled check's
    refused(call(family, name, problem(family, flags=HAS_VELOCITY), null=null, low=False), BADARG, NO_VLIM)
    # the boxes before the pass's own pointers
    refused(call(family, name, problem(family), null=null, low=False), BADARG, BOXED_ARRAYS)
    refused(call(family, name, problem(family), null=null, high=False), BADARG, BOXED_ARRAYS)


@pytest.mark.gpu
@pytest.mark.parametrize("family, name", ENTRIES, ids=IDS)
def test_own_pointers_are_checked_last(gpu, family, name):
    """A valid problem: each required pointer of the pass on its own, then all of them."""
    required = PASSES[name][1]
    for missing in [(n,) for n in required] + [required]:
        refused(call(family, name, problem(family), null=missing), BADARG, own_refusal(family, name))


@pytest.mark.gpu
@pytest.mark.parametrize("family, name", ENTRIES, ids=IDS)
def test_an_empty_batch_is_ok(gpu, family, name):
    """B = 0 with valid pointers: nothing to launch, TPR_E_OK -- with and without the optional outputs."""
    rc, msg = call(family, name, problem(family, B=0))
    assert rc == OK, (rc, msg)
    optional = tuple(n for n in PASSES[name][0] if n not in PASSES[name][1] + ("atol",))
    if optional:
        rc, msg = call(family, name, problem(family, B=0), null=optional)
        assert rc == OK, (rc, msg)
