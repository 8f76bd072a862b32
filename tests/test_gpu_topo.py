"""Topological submaps on the GPU (kernels/topo_kernels.hip, host/topo.cpp) against their numpy statement
tests/topo_model.py on the graphs of tests/_topo_cases.py.

Bars.  Eigenvalues within 1e-11 lambda_max: Jacobi stopped at off(L) <= 1e-14 ||L||_F leaves about n eps = 6e-14 at
n = 256, the bar sits two orders above.  The Fiedler vector, up to sign, within 1e-8: the eigenvalue bar over the
1e-3 lambda_max gap the cases have (the model asserts 1e-4 and a margin of 1e-6 between every entry and the mean, so
the sides cannot differ).  Cuts within 1e-12 relative: the same fp64 terms, grouped differently.  Parts, sides,
bookkeeping and the relocaliser's result are compared exactly.  Every figure is printed before it is asserted."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import rgbd360_amd as R

import _topo_cases as Cs
import topo_model as M
from test_topo_model import run_script

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = (Cs.LDS_MAX_NODES, Cs.LDS_MAX_NODES + 1)   # the last size in LDS, the first in the global scratch


@pytest.fixture(scope="module")
def ctx():
    c = R.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _ref(n, rooms):
    """A case and the model's answers, computed once: the top bisection with its figures, every bisection of the
    recursion, the parts."""
    A = Cs.case(n, rooms)
    A.setflags(write=False)
    top = {}
    s1, s2, cut = M.bisect(A, top)
    bis = M.assert_well_posed(A)
    return dict(A=A, s1=s1, s2=s2, cut=cut, top=top, bis=bis, parts=M.partition(A))


def test_sizes_cover_the_switch():
    assert R.TOPO_LDS_MAX_NODES == Cs.LDS_MAX_NODES and R.TOPO_MAX_NODES == M.MAX_NODES
    ns = [n for n, _ in Cs.SIZES]
    assert SWITCH[0] in ns and SWITCH[1] in ns and 4 in ns and 255 in ns and 256 in ns


def _rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a - b)


@pytest.mark.parametrize("n,rooms", Cs.SIZES)
def test_bisect_parity(ctx, n, rooms):
    ref = _ref(n, rooms)
    g = R.topo_bisect(ctx, ref["A"])
    w, v = ref["top"]["eigenvalues"], ref["top"]["fiedler"]
    lmax = ref["top"]["lmax"]
    d_ev = float(np.abs(g["eigenvalues"] - w).max())
    d_v = float(min(np.abs(g["fiedler"] - v).max(), np.abs(g["fiedler"] + v).max()))
    d_cut = _rel(g["cut"], ref["cut"])
    print(f"n={n}: sweeps {g['sweeps']} |d eig|/lmax {d_ev / lmax:.2e} |d fiedler| {d_v:.2e} cut {g['cut']:.15g} "
          f"rel {d_cut:.2e} margin {ref['top']['margin']:.2e} gap {ref['top']['gap']:.2e}")
    assert g["converged"] and 0 < g["sweeps"] < 40
    assert d_ev <= 1e-11 * lmax
    assert d_v <= 1e-8
    got = {frozenset(np.flatnonzero(g["side"] == 1)), frozenset(np.flatnonzero(g["side"] == 2))}
    assert got == {frozenset(ref["s1"]), frozenset(ref["s2"])}
    assert d_cut <= 1e-12


@pytest.mark.parametrize("n,rooms", Cs.SIZES)
def test_partition_parity(ctx, n, rooms):
    ref = _ref(n, rooms)
    part, cuts = R.topo_partition(ctx, ref["A"], return_cuts=True)
    want = M.part_of(ref["parts"], n)
    model_cuts = np.array([b["cut"] for b in ref["bis"]])
    print(f"n={n}: {part.max() + 1} parts (model {len(ref['parts'])}), {len(cuts)} bisections (model {len(model_cuts)})")
    assert np.array_equal(part, want)
    assert len(cuts) == len(model_cuts)
    worst = max(_rel(a, b) for a, b in zip(cuts, model_cuts))
    print(f"n={n}: worst relative cut difference {worst:.2e}")
    assert worst <= 1e-12


def _degenerate_inputs():
    out = [(f"{kind}{n}", Cs.degenerate(kind, n)) for n in (6, 65) for kind in ("zero", "cliques", "complete")]
    out.append(("one", np.zeros((1, 1), np.float32)))
    out.append(("two_apart", np.zeros((2, 2), np.float32)))
    out.append(("two_joined", np.array([[0, 0.5], [0.5, 0]], np.float32)))
    return out


@pytest.mark.parametrize("name,A", _degenerate_inputs(), ids=[k for k, _ in _degenerate_inputs()])
def test_degenerate_inputs_give_a_valid_partition(ctx, name, A):
    n = A.shape[0]
    part = R.topo_partition(ctx, A)                      # raises unless the call returns success
    n_parts = int(part.max()) + 1
    sizes = np.bincount(part, minlength=n_parts)
    firsts = [int(np.flatnonzero(part == k)[0]) for k in range(n_parts)]
    print(f"{name}: {n_parts} parts of sizes {sizes.tolist()}, first nodes {firsts}")
    assert part.min() == 0 and (sizes > 0).all()         # every node in exactly one part, every part used
    assert firsts == sorted(firsts)                      # parts ordered by their first node
    assert n_parts == 1 or (sizes >= M.MIN_CLUSTER).all()
    # the cut the hook returns is the model's ncut of the sides it returns
    g = R.topo_bisect(ctx, A)
    P, Q = list(np.flatnonzero(g["side"] == 1)), list(np.flatnonzero(g["side"] == 2))
    want = M.ncut(A, P, Q)
    print(f"{name}: sides {len(P)} | {len(Q)} cut {g['cut']:.15g} model {want:.15g} sweeps {g['sweeps']}")
    assert sorted(P + Q) == list(range(n)) and g["converged"]
    assert _rel(g["cut"], want) <= 1e-12


BATCH_SIZES = [(3, 1), (65, 5), (256, 12), (12, 3), (97, 6), (6, 2), (64, 5), (100, 6), (7, 2), (128, 8), (4, 1), (63, 5),
               (96, 6), (101, 6), (129, 8), (255, 12)]


@pytest.mark.parametrize("count", [1, 5, 16])
def test_batch_equals_lone(ctx, count):
    cases = BATCH_SIZES[:count]
    assert {3, 65, 256} <= {n for n, _ in BATCH_SIZES[:5]}
    graphs = [_ref(n, r)["A"] for n, r in cases]
    batched = R.topo_partition_batch(ctx, graphs)
    for (n, r), got in zip(cases, batched):
        lone = R.topo_partition(ctx, _ref(n, r)["A"])
        assert got.dtype == lone.dtype and got.tobytes() == lone.tobytes(), n
        assert np.array_equal(got, M.part_of(_ref(n, r)["parts"], n))


def test_the_same_call_twice_gives_the_same_bits(ctx):
    for n, r in ((65, 5), (97, 6), (256, 12)):
        A = _ref(n, r)["A"]
        a, b = R.topo_bisect(ctx, A), R.topo_bisect(ctx, A)
        for key in ("eigenvalues", "fiedler"):
            assert a[key].view(np.uint64).tobytes() == b[key].view(np.uint64).tobytes(), (n, key)
        assert a["cut"] == b["cut"] and a["sweeps"] == b["sweeps"]
        # a batch around it does not change them either: its parts equal the lone call's (test_batch_equals_lone)
        # and the cuts of a partition are those of the lone bisection at the top
        _, cuts = R.topo_partition(ctx, A, return_cuts=True)
        assert cuts[0] == a["cut"]


def test_argument_errors_are_returned(ctx):
    good = _ref(12, 3)["A"]

    def bad(**kw):
        A = good.copy()
        for (i, j), v in kw.get("set", {}).items():
            A[i, j] = v
        return A

    cases = {
        "too large": np.zeros((R.TOPO_MAX_NODES + 1,) * 2, np.float32),
        "nan": bad(set={(1, 2): np.nan, (2, 1): np.nan}),
        "inf": bad(set={(1, 2): np.inf, (2, 1): np.inf}),
        "negative": bad(set={(1, 2): -0.25, (2, 1): -0.25}),
        "asymmetric": bad(set={(1, 2): 0.75}),
        "diagonal": bad(set={(3, 3): 0.5}),
    }
    for name, A in cases.items():
        for call in (lambda: R.topo_partition(ctx, A), lambda: R.topo_bisect(ctx, A),
                     lambda: R.topo_partition_batch(ctx, [good, A])):
            with pytest.raises(RuntimeError, match=r"\(-2\)"):
                call()
        print(f"{name}: {R.lib().r360_last_error().decode()}")
    # n < 1, and parameters that make no sense
    L = R.lib()
    part, n_parts = np.zeros(4, np.int32), R.C.c_int()
    ip = R.C.POINTER(R.C.c_int)
    assert L.r360_topo_partition(ctx.h, good.ctypes.data_as(R.C.POINTER(R.C.c_float)), 0, None, part.ctypes.data_as(ip),
                                 R.C.byref(n_parts), None, None) == -2
    assert L.r360_topo_bisect(ctx.h, good.ctypes.data_as(R.C.POINTER(R.C.c_float)), -3, part.ctypes.data_as(ip), None,
                              None, None, None) == -2
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        R.topo_partition(ctx, good, R.TopoParams.default(min_cluster=0))
    # the context works afterwards
    assert np.array_equal(R.topo_partition(ctx, good), M.part_of(_ref(12, 3)["parts"], 12))


def _state(T, n_areas):
    return [T.neighbors(a) for a in range(n_areas)], [T.selected(a) for a in range(n_areas)]


def test_topological_map_follows_the_model(ctx):
    T = M.TopoMap()
    G = R.TopologicalMap(ctx)
    new_areas = []
    try:
        both = lambda f, g: (lambda *a: (f(*a), g(*a)))
        steps = run_script(None, both(T.add_keyframe, G.addKeyframe), both(T.add_connection, G.addConnection),
                           both(T.drop_last, G.dropLast), lambda: new_areas.append((T.partition(), G.Partitioner())))
        for k, step in enumerate(steps):
            area_of, n_areas, current = G.areas()
            assert list(area_of) == T.area_of and n_areas == T.n_areas and current == T.current_area, (k, step)
            assert _state(G, n_areas) == _state(T, n_areas), (k, step)
            ids, A = G.getVicinitySSO()
            kfs, B = T.vicinity()
            assert list(ids) == kfs and np.array_equal(A, B), (k, step)
        print(f"new areas per cut (model, library): {new_areas}; areas {T.area_of}; current {T.current_area}; "
              f"neighbours and representatives {_state(T, T.n_areas)}")
        assert new_areas == [(2, 2), (0, 0), (0, 0)] and T.n_areas == 3
    finally:
        G.close()


SEED = 360 << 16
PATH_INDICES = (0, 4, 8, 12, 16)


@pytest.fixture(scope="module")
def keyframes():
    """Keyframes at the path indices tests/test_gpu_kfsphere_slam.py walks, and a query frame at one of them."""
    c = R.Context(0)
    cal = R.Calib360(c, 480, 640)
    cal.loadExtrinsicCalibration(R.EXTRINSICS_DIR)

    def frame(index):
        b, d = cal.synth_frame(SEED, R.synth_path_pose(SEED, index))
        f = R.Frame360(cal)
        f.upload(b, d)
        f.build(R.BUILD_UNDISTORT | R.BUILD_CLOUD | R.BUILD_PLANES)
        return f

    kfs = [frame(i) for i in PATH_INDICES]
    query = frame(8)
    yield dict(ctx=c, kfs=kfs, query=query)
    for f in kfs + [query]:
        f.close()
    cal.close()
    c.close()


def _sequential(ctx, kfs, query, min_matches, min_area):
    """Relocalizer360.h:80-90 with RegisterRGBD360.RegisterPbMap: (index or -1, pose, information)."""
    reg = R.RegisterRGBD360(ctx)
    for i in range(len(kfs) - 1, -1, -1):
        ok = reg.RegisterPbMap(kfs[i], query, 25, R.PLANAR_3DoF)
        print(f"keyframe {i}: {'ok' if ok else 'failed'} matches {len(reg.getMatchedPlanes())} area {reg.getAreaMatched():.3f}")
        if ok and len(reg.getMatchedPlanes()) >= min_matches and reg.getAreaMatched() > min_area:
            return i, reg.getPose().astype(np.float64), reg.getInfoMat().astype(np.float64)
    return -1, None, None


@pytest.mark.parametrize("lanes", [1, 4])
def test_relocalizer_equals_the_sequential_loop(keyframes, lanes):
    """The reference's gates (5 planes, 10 m2), and two stricter pairs that send the loop past the newest keyframes
    (and past a chunk of lanes): whatever the sequential loop answers under the same gates, the library answers."""
    kfs, query = keyframes["kfs"], keyframes["query"]
    batch = R.Batch(0, lanes=lanes)
    try:
        for min_matches, min_area in ((5, 10.0), (17, 10.0), (5, 165.0)):
            want, pose, info = _sequential(keyframes["ctx"], kfs, query, min_matches, min_area)
            rel = R.Relocalizer(batch, min_matches=min_matches, min_area=min_area)
            got = rel.relocalize(kfs, query)
            print(f"lanes {lanes}, gates {min_matches} / {min_area}: relocalised against {got} (sequential loop: {want})")
            assert got == want
            if want >= 0:
                assert rel.relocKF == want
                assert rel.rigidTransf.tobytes() == pose.tobytes()
                assert rel.informationM.tobytes() == info.tobytes()
            else:
                assert min_matches != 5 or min_area != 10.0   # under the reference's gates the frame is found
        assert R.Relocalizer(batch, min_matches=1000).relocalize(kfs, query) == -1
        assert R.Relocalizer(batch).relocalize([], query) == -1
    finally:
        batch.close()


def test_kfsphere_slam_with_submaps():
    exe = os.path.join(ROOT, "build", "bin", "KFsphereSLAM")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build()"
    p = subprocess.run([exe, "--synthetic-frames", "0,4,8,12,16,12,8,4,0", "1", "--submaps"], capture_output=True,
                       text=True, timeout=100)
    assert p.returncode == 0, p.stderr + p.stdout[-2000:]
    out = p.stdout
    n_kf = int(re.search(r"(\d+) keyframes, \d+ loop edges", out).group(1))
    places = re.search(r"^\tPlaces\n((?:\t\d+:(?: \d+)*\n)+)", out, re.M)
    assert places, out[-3000:]
    print(places.group(0))
    print(re.findall(r"^SSO is \S+$", out, re.M))
    areas = re.findall(r"^area (\d+): keyframes((?: \d+)*) representative (\d+)( current)?$", out, re.M)
    print(areas)
    assert areas and [int(a[0]) for a in areas] == list(range(len(areas)))
    seen = sorted(int(k) for a in areas for k in a[1].split())
    assert seen == list(range(n_kf))                     # every keyframe in exactly one area
    for _, kf_list, rep, _ in areas:
        assert not kf_list.split() or rep in kf_list.split()
    assert sum(1 for a in areas if a[3]) == 1
