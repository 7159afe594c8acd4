"""The box-limit builder of the rigid-body constraints without a GPU (``toppra_amd.constraint._box_limits``): the rows five
constructors get from it -- ``con.F``, ``con.g``, ``con._limit_batch`` -- against rows written out here entry by entry, at the
smallest inputs where the layout can go wrong, and the two refusals that carry each family's words.  The layout: rows are
unit-major (a unit = the tool point, the one wrench, a section, a control point); within a unit the parts follow in their order
(linear before angular, force before moment); each part is [+I; -I] on its three columns with g = [upper; -lower]."""
import numpy as np
import pytest

from toppra_amd.chain import ControlPoints, JointSections, Mount, Payload, SerialChain
from toppra_amd.constraint import (BatchBaseWrenchConstraint, BatchCartesianAccelerationConstraint, BatchJointLoadConstraint,
                                   BatchPointAccelerationConstraint, BatchToolWrenchConstraint)

CHAIN = SerialChain(["r", "p", "r"], [[0.0, 0.0, 1.0]] * 3, [np.eye(3)] * 3, [[0.0, 0.0, 0.1], [0.2, 0.0, 0.0], [0.0, 0.3, 0.0]],
                    [1.0, 2.0, 0.5], np.zeros((3, 3)), np.tile([0.1, 0.1, 0.1, 0.0, 0.0, 0.0], (3, 1)))


def _bounds(lead, tag):
    """(lower, upper) [*lead, 3, 2], no two entries alike -- here or in another part (``tag``) -- and lower < upper."""
    n = int(np.prod(lead + (3,)))
    upper = (tag + 1.0 + np.arange(n) / 64.0).reshape(lead + (3,))
    return np.stack([-2.0 * upper, upper], -1)


def _expect(count, width, parts, B=None):
    """(F, g) written out by index.  ``parts``: (first column in a unit, bound(b, k, i) -> (lower, upper)) of each part that is
    given, in order; ``B``: the trajectories of limits given per trajectory."""
    per = 6 * len(parts)
    F = np.zeros((per * count, width * count))
    g = np.zeros((() if B is None else (B,)) + (per * count,))
    for k in range(count):
        for j, (at, bound) in enumerate(parts):
            for i in range(3):
                up, down, col = per * k + 6 * j + i, per * k + 6 * j + 3 + i, width * k + at + i
                F[up, col], F[down, col] = 1.0, -1.0
                for b in range(1 if B is None else B):
                    lower, upper = bound(b, k, i)
                    if B is None:
                        g[up], g[down] = upper, -lower
                    else:
                        g[b, up], g[b, down] = upper, -lower
    return F, g


def _same(con, F, g, B):
    assert con.F.dtype == con.g.dtype == np.float64 and con.g.flags.c_contiguous
    assert np.array_equal(con.F, F) and np.array_equal(con.g, g) and con._limit_batch == B
    assert con.rows_per_stage(3) == 2 * F.shape[0]  # (Interpolation: two gridpoints' rows per stage)


# the three constructors on one 6-wide unit, and their names for its two parts
SIX = {"accel": (lambda **kw: BatchCartesianAccelerationConstraint(CHAIN, **kw), "linear", "angular"),
       "tool": (lambda **kw: BatchToolWrenchConstraint(CHAIN, Payload(1.0), **kw), "force", "moment"),
       "base": (lambda **kw: BatchBaseWrenchConstraint(CHAIN, Mount(), **kw), "force", "moment")}
SECTIONS = JointSections([0, 2])
POINTS = ControlPoints([1, 2], [[0.0, 0.0, 0.1], [0.1, 0.0, 0.0]])


@pytest.mark.parametrize("family", sorted(SIX))
def test_one_unit_with_only_its_second_part_sits_at_column_three(family):
    make, _, second = SIX[family]
    box = _bounds((), 0)
    _same(make(**{second: box}), *_expect(1, 6, [(3, lambda b, k, i: box[i])]), None)
    _same(make(**{second: 2.5}), *_expect(1, 6, [(3, lambda b, k, i: (-2.5, 2.5))]), None)


@pytest.mark.parametrize("family", sorted(SIX))
def test_one_unit_with_both_parts_and_one_of_them_per_trajectory(family):
    make, first, second = SIX[family]
    one, each = _bounds((), 0), _bounds((2,), 8)
    _same(make(**{first: one, second: one + 4.0}), *_expect(1, 6, [(0, lambda b, k, i: one[i]), (3, lambda b, k, i: one[i] + 4.0)]), None)
    _same(make(**{first: each, second: one}), *_expect(1, 6, [(0, lambda b, k, i: each[b, i]), (3, lambda b, k, i: one[i])], 2), 2)
    _same(make(**{first: 1.5, second: each}), *_expect(1, 6, [(0, lambda b, k, i: (-1.5, 1.5)), (3, lambda b, k, i: each[b, i])], 2), 2)


def test_two_sections_interleave_force_and_moment_within_each_section():
    force, moment = _bounds((2,), 0), _bounds((2,), 16)
    both = [(0, lambda b, k, i: force[k, i]), (3, lambda b, k, i: moment[k, i])]
    _same(BatchJointLoadConstraint(CHAIN, SECTIONS, force=force, moment=moment), *_expect(2, 6, both), None)
    _same(BatchJointLoadConstraint(CHAIN, SECTIONS, moment=moment), *_expect(2, 6, both[1:]), None)
    _same(BatchJointLoadConstraint(CHAIN, SECTIONS, force=force), *_expect(2, 6, both[:1]), None)


def test_two_sections_with_one_part_per_trajectory_beside_a_shared_one():
    force, moment = _bounds((2, 2), 0), _bounds((2,), 16)
    _same(BatchJointLoadConstraint(CHAIN, SECTIONS, force=force, moment=moment),
          *_expect(2, 6, [(0, lambda b, k, i: force[b, k, i]), (3, lambda b, k, i: moment[k, i])], 2), 2)
    _same(BatchJointLoadConstraint(CHAIN, SECTIONS, force=moment, moment=force),
          *_expect(2, 6, [(0, lambda b, k, i: moment[k, i]), (3, lambda b, k, i: force[b, k, i])], 2), 2)


def test_a_magnitude_per_unit():
    _same(BatchJointLoadConstraint(CHAIN, SECTIONS, force=[3.0, 5.0], moment=7.0),
          *_expect(2, 6, [(0, lambda b, k, i: (-(3.0, 5.0)[k], (3.0, 5.0)[k])), (3, lambda b, k, i: (-7.0, 7.0))]), None)
    _same(BatchPointAccelerationConstraint(CHAIN, POINTS, linear=[3.0, 5.0]), *_expect(2, 3, [(0, lambda b, k, i: (-(3.0, 5.0)[k], (3.0, 5.0)[k]))]), None)
    # one unit has no such spelling: [1] is no box
    with pytest.raises(ValueError, match=r"^force must be a scalar or have shape \[3, 2\] or \[B, 3, 2\], got \[1\]$"):
        BatchBaseWrenchConstraint(CHAIN, force=[3.0])


def test_two_points_are_three_wide():
    box, each = _bounds((2,), 0), _bounds((2, 2), 8)
    _same(BatchPointAccelerationConstraint(CHAIN, POINTS, linear=box), *_expect(2, 3, [(0, lambda b, k, i: box[k, i])]), None)
    _same(BatchPointAccelerationConstraint(CHAIN, POINTS, linear=each), *_expect(2, 3, [(0, lambda b, k, i: each[b, k, i])], 2), 2)
    _same(BatchPointAccelerationConstraint(CHAIN, POINTS, linear=4.0), *_expect(2, 3, [(0, lambda b, k, i: (-4.0, 4.0))]), None)


def test_two_parts_per_trajectory_for_different_batches_are_refused():
    for family, (make, first, second) in sorted(SIX.items()):
        with pytest.raises(ValueError, match="^%s and %s are given per trajectory for 2 and 3 trajectories$" % (first, second)):
            make(**{first: _bounds((2,), 0), second: _bounds((3,), 0)})
    with pytest.raises(ValueError, match="^force and moment are given per trajectory for 3 and 2 trajectories$"):
        BatchJointLoadConstraint(CHAIN, SECTIONS, force=_bounds((3, 2), 0), moment=_bounds((2, 2), 0))


ALL = dict(SIX, load=(lambda **kw: BatchJointLoadConstraint(CHAIN, SECTIONS, **kw), "force", "moment"),
           points=(lambda **kw: BatchPointAccelerationConstraint(CHAIN, POINTS, **kw), "linear", None))


@pytest.mark.parametrize("family", sorted(ALL))
def test_boxes_beside_rows_and_no_limit_at_all_are_refused_in_the_family_s_words(family):
    make, first, second = ALL[family]
    width = {"load": 12, "points": 6}.get(family, 6)
    names = "%s / %s" % (first, second) if second else first
    with pytest.raises(ValueError, match="^give the limits either as %s or as F and g, not both$" % names):
        make(**{first: 1.0, "F": np.ones((1, width)), "g": np.ones(1)})
    with pytest.raises(ValueError, match="^give the limits either as %s or as F and g, not both$" % names):
        make(**{second or first: 1.0, "g": np.ones(1)})
    missing = "one of %s, %s, or F with g, is required" % (first, second) if second else "%s, or F with g, is required" % first
    with pytest.raises(ValueError, match="^no limit given: %s$" % missing):
        make()
