"""The numpy statement of the topological submaps (tests/topo_model.py) on hand-computed graphs, the conditions the
generated parity cases (tests/_topo_cases.py) must satisfy, the bookkeeping on the scripted 12-keyframe run, and the
façade's call-site file.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import _topo_cases as Cs
import topo_model as M


def _graph(n, edges):
    A = np.zeros((n, n), np.float32)
    for i, j, w in edges:
        A[i, j] = A[j, i] = w
    return A


def test_two_triangles_split_at_the_weak_edge():
    tri = [(0, 1, 1), (0, 2, 1), (1, 2, 1)]
    A = _graph(6, tri + [(i + 3, j + 3, w) for i, j, w in tri] + [(2, 3, 0.1)])
    s1, s2, cut = M.bisect(A)
    assert {frozenset(s1), frozenset(s2)} == {frozenset({0, 1, 2}), frozenset({3, 4, 5})}
    assert cut == pytest.approx(0.1 / 3.1 * 2, rel=1e-7)   # the weight 0.1 is an fp32 value
    assert M.partition(A) == [[0, 1, 2], [3, 4, 5]]
    assert list(M.part_of(M.partition(A), 6)) == [0, 0, 0, 1, 1, 1]


def test_path_p4_fiedler_split():
    A = _graph(4, [(0, 1, 1), (1, 2, 1), (2, 3, 1)])
    info = {}
    s1, s2, cut = M.bisect(A, info)
    assert {frozenset(s1), frozenset(s2)} == {frozenset({0, 1}), frozenset({2, 3})}
    assert info["eigenvalues"] == pytest.approx([0, 2 - np.sqrt(2), 2, 2 + np.sqrt(2)], abs=1e-12)
    assert cut == pytest.approx(1 / 2 + 1 / 2)


def test_ncut_by_hand():
    #   0 -2- 1
    #   |3    |1      P = {0, 2}, Q = {1, 3}: across a01 + a23 = 2 + 4, inside P a02 = 3, inside Q a13 = 1
    #   2 -4- 3
    A = _graph(4, [(0, 1, 2), (0, 2, 3), (1, 3, 1), (2, 3, 4)])
    c, aa, bb = 2.0 + 4.0, 3.0, 1.0
    assert M.ncut(A, [0, 2], [1, 3]) == pytest.approx(c / (aa + c) + c / (bb + c), rel=1e-15)
    # the diagonal counts among the inside edges
    B = A.copy()
    B[0, 0] = 5
    assert M.ncut(B, [0, 2], [1, 3]) == pytest.approx(c / (aa + 5 + c) + c / (bb + c), rel=1e-15)
    # no edge across: 0, whatever is inside
    D = _graph(4, [(0, 2, 3), (1, 3, 1)])
    assert M.ncut(D, [0, 2], [1, 3]) == 0.0
    assert M.ncut(A, [0, 1, 2, 3], []) == 0.0


def test_empty_side_fallback():
    for n in (1, 2, 5, 6):
        s1, s2 = M.sides_of(np.full(n, 0.25))     # every v_i >= mean: side 2 would be empty
        assert s1 == [i for i in range(n) if i <= n // 2] and s2 == [i for i in range(n) if i > n // 2]
    s1, s2 = M.sides_of(np.array([np.nan, 1.0, 2.0]))   # no v_i >= mean: side 1 would be empty
    assert s1 == [0, 1] and s2 == [2]
    # a single node: the fallback, a zero cut, one part
    s1, s2, cut = M.bisect(np.zeros((1, 1), np.float32))
    assert (s1, s2, cut) == ([0], [], 0.0)
    assert M.partition(np.zeros((1, 1), np.float32)) == [[0]]


def test_small_clusters_and_the_threshold_stop_the_recursion():
    tri = [(0, 1, 1), (0, 2, 1), (1, 2, 1)]
    A = _graph(6, tri + [(i + 3, j + 3, w) for i, j, w in tri] + [(2, 3, 0.1)])
    assert M.partition(A, min_cluster=4) == [[0, 1, 2, 3, 4, 5]]
    assert M.partition(A, threshold=0.01) == [[0, 1, 2, 3, 4, 5]]
    bis = []
    M.partition(A, bisections=bis)
    assert [len(b["nodes"]) for b in bis] == [6, 3, 3] and [b["split"] for b in bis] == [True, False, False]


@pytest.mark.parametrize("n,rooms", Cs.SIZES)
def test_generated_cases_are_well_posed(n, rooms):
    """Every bisection of every parity case: margin >= 1e-6, gap >= 1e-4 lambda_max, |cut - 0.8| >= 1e-6; the parts are
    a partition into clusters of at least 3 nodes."""
    A = Cs.case(n, rooms)
    assert A.dtype == np.float32 and np.array_equal(A, A.T) and not A.diagonal().any() and (A >= 0).all()
    bis = M.assert_well_posed(A)
    parts = M.partition(A)
    print(f"n={n} rooms={rooms} seed={Cs.seed_of(n, rooms)}: {len(parts)} parts, {len(bis)} bisections, "
          f"margin {min(b['margin'] for b in bis):.2e} gap {min(b['gap'] for b in bis):.2e} "
          f"|cut-0.8| {min(abs(b['cut'] - 0.8) for b in bis):.2e}")
    assert sorted(i for p in parts for i in p) == list(range(n))
    assert 1 <= len(parts) <= 26 and all(len(p) >= 3 for p in parts)
    assert [p[0] for p in parts] == sorted(p[0] for p in parts)


def run_script(T, add_kf, conn, drop, cut):
    """Drives a map through Cs.scripted_run() and yields after every step."""
    for step in Cs.scripted_run():
        if step[0] == "kf":
            add_kf()
        elif step[0] == "conn":
            conn(*step[1:])
        elif step[0] == "drop":
            drop()
        else:
            cut()
        yield step


def test_bookkeeping_on_the_scripted_run():
    T = M.TopoMap()
    cuts = []
    snapshots = []
    for step in run_script(T, T.add_keyframe, T.add_connection, T.drop_last, lambda: cuts.append(T.partition())):
        if step[0] == "drop":
            assert (11, 12) not in T.sso and len(T.area_of) == 12
        if step[0] in ("cut", "drop"):
            snapshots.append((list(T.area_of), T.current_area, [T.neighbors(a) for a in range(T.n_areas)],
                              [T.selected(a) for a in range(T.n_areas)]))
    # the first cut turns the one area into three; the second finds nothing to do (k <= 0)
    assert cuts == [2, 0, 0]
    three = [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]
    assert snapshots[0] == (three, 2, [[0, 1], [0, 1, 2], [1, 2]], [1, 5, 9])
    assert snapshots[1] == snapshots[0]
    # keyframe 12 was added to the current area and dropped again, with its connection
    assert snapshots[2] == snapshots[0]
    # keyframe 12 joins area 2; its connection to keyframe 1 makes areas 0 and 2 neighbours; the last cut has as many
    # parts as the vicinity has areas at most, so nothing moves; the representative of area 2 is now keyframe 10
    assert snapshots[3] == (three + [2], 2, [[0, 1, 2], [0, 1, 2], [0, 1, 2]], [1, 5, 10])
    # the vicinity lists the areas ascending and their keyframes ascending
    kfs, A = T.vicinity()
    assert kfs == list(range(13)) and A.shape == (13, 13) and A[1, 12] == np.float32(0.3) and A[12, 1] == A[1, 12]


def test_vicinity_leaves_out_areas_that_are_not_neighbours():
    T = M.TopoMap()
    for step in run_script(T, T.add_keyframe, T.add_connection, T.drop_last, T.partition):
        if step[0] == "cut":
            break
    # after the first cut the current area is 2, whose only neighbour is 1
    assert T.current_area == 2 and T.neighbors(2) == [1, 2]
    kfs, A = T.vicinity()
    assert kfs == [4, 5, 6, 7, 8, 9, 10, 11] and A.shape == (8, 8)
    # fewer than three keyframes in the vicinity: nothing happens
    S = M.TopoMap()
    S.add_keyframe(); S.add_keyframe()
    S.add_connection(0, 1, 0.5)
    assert S.partition() == 0 and S.area_of == [0, 0]


def test_topological_map_call_sites_compile(root):
    """Source-level drop-in: tests/dropin/topological_map_dropin.cpp makes the reference's Map360 /
    TopologicalMap360 / Relocalizer360 calls with its constructors, with g++ alone."""
    p = subprocess.run(["g++", "-std=c++17", "-O0", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", f"-I{root}/include",
                        f"{root}/tests/dropin/topological_map_dropin.cpp"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


def test_app_with_submaps_compiles_with_gxx_alone(root):
    p = subprocess.run(["g++", "-std=c++17", "-O0", "-fsyntax-only", "-Wall", "-Werror", f"-I{root}/include",
                        f'-DRGBD360_DATA_DIR="{root}/data"', f"{root}/apps/KFsphereSLAM.cpp"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "--submaps" in open(os.path.join(root, "apps", "KFsphereSLAM.cpp")).read()
