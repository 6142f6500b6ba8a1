"""The Morison strip members at the edges of their launches (csrc/hc_morison_members.hip): both sum levels across a workgroup edge of
256 rows, grids whose last workgroup is partly filled or exactly full, and nodes exactly on the free surface.  Values are held to
tests/morison_members_ref.py inside the bounds it derives, per body and per member (compare() of tests/test_gpu_morison_members.py);
the surface nodes, which that restatement rightly refuses (the wet test is a discontinuity there), to closed forms at the rtol = 1e-13
of that file's closed-form test.  The inputs are fixed in tests/morison_members_inputs.py; tests/test_morison_members_inputs_cpu.py
asserts their conditions on the CPU, compare() again on the context's own spectrum."""
import time

import numpy as np
import pytest

import morison_members_inputs as mi
from cases import sphere_case
from test_gpu_morison_members import HF, compare, same_bits, set_all  # noqa: F401

pytestmark = pytest.mark.gpu


def edge_context(HF, case, body_range=None):
    h = HF.from_case(case, body_range=body_range)
    h.add_waves_irregular(spectral=True, **mi.EDGE_SEA)
    h.set_morison_options(**mi.EDGE_OPTS)
    return h


def held(h, case, lists, state, what, need, heading=None):
    comp = mi.edge_components(h, heading)
    assert comp[0].size == 64
    return compare(h, case, lists, comp, mi.EDGE_T, state, what, mwl=mi.EDGE_OPTS["mwl"], stretching=True,
                   ramp=1.0, need=need)


# ------------------------------------------------------------------------------------------------
# 1: the sum kernels across a workgroup edge
# ------------------------------------------------------------------------------------------------
def test_level_one_sum_across_a_workgroup_edge(HF):
    """50 members of 1, 2, 3, 5, 4 segments: 300 rows of the first sum level in two workgroups, an irregular first-segment list"""
    case = sphere_case()
    h = edge_context(HF, case)
    lists = mi.edge_lists()
    set_all(h, lists)
    assert h.morison_member_count(0) == 50 and mi.counts(lists[0]) == (50, 200, 300)
    got, ref = held(h, case, lists, mi.edge_state(), "50 members", mi.ALL_CASES)
    rows = h.morison_member_forces(0)
    assert rows.shape == (50, 6) and np.abs(got).max() > 100.0
    # member 42 owns rows 252..257, on both sides of row 256: it and a member behind it carry a force; a dry member is exact zeros
    wet = [m for m in range(50) if ref["members"][0][m].any()]
    assert 42 in wet and 44 in wet and len(wet) < 50
    assert all(same_bits(rows[m], np.zeros(6)) for m in range(50) if m not in wet)
    h.close()


def test_level_two_sum_across_a_workgroup_edge(HF):
    """48 bodies: Dloc = 288 rows of the second sum level; bodies 42 and 43 own rows 252..263.  The invariant of DESIGN 3.7c': a
    body's bits depend on its own state and list, not on the other bodies or the shard."""
    t0 = time.perf_counter()
    case = mi.many_case()
    h = edge_context(HF, case)
    print(f"48 bodies: context set up in {time.perf_counter() - t0:.2f} s")
    lists = mi.many_lists()
    set_all(h, lists)
    st = mi.many_state()
    assert h.D_local == 288
    # the restatement for the five bodies only: a 5-body problem with their states
    idx = list(mi.MANY_BODIES)
    comp = mi.edge_components(h, None)
    sub = [np.asarray(x).reshape(-1, 3)[idx] for x in st]
    ref = mi.restate(case, [lists[b] for b in idx], comp, mi.EDGE_T, sub, mi.EDGE_OPTS, mi.EDGE_SEA["ramp_duration"], True)
    mi.check_conditions(ref, "48 bodies", mi.ALL_CASES)
    got = h.compute_morison(mi.EDGE_T, *st).reshape(-1, 6)
    assert got.shape == (48, 6) and np.all(np.isfinite(got))
    worst = 0.0
    for i, b in enumerate(idx):
        rows = h.morison_member_forces(b)
        err, merr = np.abs(got[b] - ref["F"][i]), np.abs(rows - ref["members"][i])
        worst = max(worst, float(np.max(err / ref["bound"][i])), float(np.max(merr / np.maximum(ref["member_bound"][i], 1e-300))))
        assert np.all(err <= ref["bound"][i]) and np.all(merr <= ref["member_bound"][i]), b
        assert got[b].any()
    print(f"48 bodies: worst |gpu - ref| / bound = {worst:.3e} (body vectors and member rows)")
    for b in range(48):
        if b not in idx:
            assert same_bits(got[b], np.zeros(6)), b
    # bodies 42 and 43 alone in a one-body context, and in the shard of bodies 40..47
    shard = edge_context(HF, case, body_range=mi.MANY_SHARD)
    set_all(shard, lists)
    gs = shard.compute_morison(mi.EDGE_T, *st).reshape(-1, 6)
    assert same_bits(gs, got[mi.MANY_SHARD[0]:mi.MANY_SHARD[1]])
    one = edge_context(HF, mi.many_case(1))
    for b in (42, 43):
        assert same_bits(shard.morison_member_forces(b), h.morison_member_forces(b))
        one.set_morison_members(0, *lists[b])
        g1 = one.compute_morison(mi.EDGE_T, *[np.asarray(x).reshape(-1, 3)[b] for x in st])
        assert same_bits(g1, got[b]) and same_bits(one.morison_member_forces(0), h.morison_member_forces(b)), b
    for x in (h, shard, one):
        x.close()
    print(f"48 bodies: whole test {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------------------------------------
# 2: nodes exactly on the surface, still water
# ------------------------------------------------------------------------------------------------
def still(HF, nowave):
    h = HF.from_case(sphere_case())
    if nowave:
        h.add_waves_none()
    return h


def surge(h, z):
    return h.compute_morison(0.0, [0.0, 0.0, z], np.zeros(3), [mi.SURF_U, 0.0, 0.0], np.zeros(3))


@pytest.mark.parametrize("nowave", [False, True])
def test_nodes_exactly_on_the_surface(HF, nowave):
    case = sphere_case()
    h = still(HF, nowave)
    per_m = -0.5 * case["rho"] * mi.SURF_CD * mi.SURF_D * mi.SURF_U ** 2  # drag per metre of draft on the surging body
    for top_down in (False, True):  # top down: the wet interval is [1 - cut, 1] with cut = -0.0
        for n_seg in (2, 4):  # the middle node sits exactly in the surface: wet, with a dry neighbour
            h.set_morison_members(0, *mi.surface_column(n_seg, top_down))
            for mwl, z in ((0.0, 0.0), (0.5, 0.5)):
                h.set_morison_options(mwl=mwl)
                got = surge(h, z)
                rows = h.morison_member_forces(0)
                assert np.all(np.isfinite(got)) and np.all(np.isfinite(rows)), (top_down, n_seg, mwl)
                assert np.isclose(got[0], per_m * 4.0, rtol=1e-13) and same_bits(rows[0], got), (top_down, n_seg, mwl, got[0], per_m * 4.0)
                # the uniform load of 4 m of draft acts 2 m below the surface; the arm is measured from the body reference at z
                assert np.isclose(got[4], -2.0 * per_m * 4.0, rtol=1e-13) and not got[[1, 2, 3, 5]].any()
    # a horizontal member lying in the surface: every h_j is exactly zero, wet over its whole length
    h.set_morison_options(mwl=0.0)
    sway = (lambda z: h.compute_morison(0.0, [0.0, 0.0, z], np.zeros(3), [0.0, mi.SURF_U, 0.0], np.zeros(3)))
    for n_seg in (1, 3):
        h.set_morison_members(0, *mi.surface_beam(n_seg))
        got = sway(0.0)
        assert np.isclose(got[1], per_m * 8.0, rtol=1e-13) and np.all(np.isfinite(got)), (n_seg, got)
        # The yaw moment of the symmetric load is zero but for rounding: part 3 of the restatement's bound, (items + 64) 2^-52 of the
        # magnitude without cancellation, with items = 2 n_seg points and the magnitude |F_y| times the largest arm, 4 m
        assert not got[[0, 2, 3, 4]].any() and abs(got[5]) <= (2 * n_seg + 64) * mi.mm.EPS * 4.0 * abs(got[1]), (n_seg, got)
        # one ulp higher it is dry: six exact zeros
        up = sway(np.nextafter(0.0, 1.0))
        assert same_bits(up, np.zeros(6)) and same_bits(h.morison_member_forces(0), np.zeros((1, 6))), (n_seg, up)
    h.close()


# ------------------------------------------------------------------------------------------------
# 3: grid tails
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heading", [None, mi.EDGE_HEADING])
def test_grid_tails(HF, heading):
    """2 nodes, 2 points and 6 rows in one partly filled workgroup each; then exactly 256 nodes; then exactly 512 points -- in the
    long-crested and the directional instantiation of the kernels"""
    case = sphere_case()
    h = edge_context(HF, case)
    if heading is not None:
        th = h.set_wave_spreading(heading, s=0.0)
        assert np.all(th == heading) and h.wave_directions().size == 64
    results = []
    for name, (ml, need) in mi.tail_lists().items():
        h.set_morison_members(0, *ml)
        got, _ = held(h, case, [ml], mi.edge_state(), f"tails: {name}, heading {heading}", need, heading)
        assert got.any()
        results.append(got)
    assert not same_bits(results[1], results[2])
    h.close()
