"""The tick schedule of the staged fvDOM ray sweep (csrc/ffm_rays.cpp: ffm_ray_schedule, host code): on a box of blocks every
(ray, block) pair is solved exactly once, every upstream face neighbour of a block has solved the ray in an earlier tick (so its
values are in the ghost cells when the block needs them), every block computes the same number of ticks (so a sweep that enters
one exchange per tick cannot hang) and no block has two rays in a tick."""
import itertools

import numpy as np
import pytest

GRIDS = [(1, 1, 1), (2, 1, 1), (1, 2, 1), (2, 2, 1), (2, 2, 2), (3, 2, 1)]


def default_rays():
    """the driver's default ray set, nPhi 2, nTheta 4 -> 32 rays (fvDOM.C:55-90, as ffm_plume_set_radiation builds them)"""
    nPhi, nTheta = 2, 4
    dPhi, dTheta = np.pi / (2.0 * nPhi), np.pi / nTheta
    d = []
    for n in range(1, nTheta + 1):
        for m in range(1, 4 * nPhi + 1):
            theta, phi = (2.0 * n - 1.0) * dTheta / 2.0, (2.0 * m - 1.0) * dPhi / 2.0
            a = np.sin(0.5 * dPhi) * (dTheta - np.cos(2.0 * theta) * np.sin(dTheta))
            d.append([np.sin(phi) * a, np.cos(phi) * a, 0.5 * dPhi * np.sin(2.0 * theta) * np.sin(dTheta)])
    return np.array(d)


def user_rays():
    """a user ray set with direction components of exactly 0 and of -0.0 (both count as positive: w = 1 where d & Sf >= 0),
    octants of different sizes and empty octants"""
    return np.array([[0.3, 0.0, 0.2], [0.0, -0.4, 0.1], [-0.0, 0.5, -0.2], [-0.3, -0.0, 0.6], [0.2, 0.1, -0.0],
                     [-0.1, -0.2, -0.3], [0.0, 0.0, 1.0], [-0.5, 0.25, 0.0], [0.4, 0.4, 0.4]])


RAYS = {"default32": default_rays(), "user": user_rays()}


def octant(d):
    return int(d[0] < 0) | int(d[1] < 0) << 1 | int(d[2] < 0) << 2


def test_octant_uses_the_sign_rule_of_the_upwind_weights(ffm):
    for d in itertools.chain(default_rays(), user_rays()):
        assert ffm.ray_octant(d) == octant(d)
    assert ffm.ray_octant(np.array([-0.0, 0.0, -0.0])) == 0
    assert len(default_rays()) == 32 and sorted(np.bincount([octant(d) for d in default_rays()], minlength=8)) == [4] * 8


@pytest.mark.parametrize("rays", sorted(RAYS))
@pytest.mark.parametrize("grid", GRIDS)
def test_schedule(ffm, grid, rays):
    d = RAYS[rays]
    nRay = len(d)
    blocks = list(itertools.product(range(grid[0]), range(grid[1]), range(grid[2])))
    sched = {b: ffm.ray_schedule(grid, b, d) for b in blocks}
    # the tick count is the same from every block's call and is the sum over the octants that have rays of rays + stages - 1
    stages = sum(g - 1 for g in grid) + 1
    perOct = np.bincount([octant(x) for x in d], minlength=8)
    expected = int(sum(r + stages - 1 for r in perOct if r > 0))
    assert {n for _, n in sched.values()} == {expected}
    tickOf = {}
    for b, (ticks, n) in sched.items():
        assert len(ticks) == n
        solved = ticks[ticks >= 0]
        # a block never has two rays in one tick (a tick names one ray or none), and every (ray, block) pair occurs exactly once
        assert sorted(solved.tolist()) == list(range(nRay)), (b, ticks)
        for t, r in enumerate(ticks):
            if r >= 0:
                assert (int(r), b) not in tickOf
                tickOf[(int(r), b)] = t
    assert len(tickOf) == nRay * len(blocks)
    # every upstream face neighbour of a block solves the same ray at a strictly earlier tick
    for (r, b), t in tickOf.items():
        for a in range(3):
            up = list(b)
            up[a] += 1 if d[r][a] < 0 else -1          # rays that run along +a come from the block below
            if 0 <= up[a] < grid[a]:
                assert tickOf[(r, tuple(up))] < t, (r, b, up)
    # octants follow one another in index order, rays of an octant in ray-index order on every block
    for b, (ticks, _) in sched.items():
        order = [int(r) for r in ticks if r >= 0]
        assert order == sorted(order, key=lambda r: (octant(d[r]), r))
