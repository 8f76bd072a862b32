"""k_match_tables and RegisterPbMap on crafted plane maps (tests/_match_cases.py), on the GPU.  Frames are made by
Frame360.loadPbMap of files written by oracle/persist_oracle.py's pbmap_bytes; no image is uploaded or built.

* the tables (sid, tid, unary, binary) equal the oracle's bit for bit for every case, every registration mode and both
  threshold sets (table shapes with ns * nt of 63 / 64 / 65, two words, lopsided maps, 70 x 66; every comparison at
  thr (1 -+ 2^-10) and exactly on its threshold; selection with ties and curved planes; a NaN plane), padding bits are
  zero, and they equal the float64 model (tests/match_model.py) on all its decided entries; a large table before the
  small ones on one context, and the same bytes again on a fresh context;
* RegisterPbMap equals the oracle's (verdict, matches, areas, pose and information bit for bit, no truncation), the
  model's pose and the construction's G within the north-star bar (1e-4 rad, 1e-3 m), the model's information within
  2^-22 relative (the float32 store of a float64 sum accounts for 2^-24);
* a failed call leaves pose, information and areas untouched; 16 jobs over a 4-lane Batch equal the lone calls;
  save / load / save reproduces the writer's bytes; a file whose plane ids are not 0..n-1 is refused.

Measured on an MI355X (printed with -s; recorded here, not asserted): pose against G at most 2.20e-08 rad and
2.27e-07 m, against the model 2.56e-08 rad and 2.03e-08 m; information against the model 3.80e-08 relative at most;
the NaN plane is matched (6 matches) and the registration fails, in the library as in the oracle; 0.0217 % of the
196 M table entries are undecided by the model.  The whole file takes 5.2 s.

What a wrong kernel does to this file (scratch builds, one change each): without `&& l != j` the `twins` case fails
test_tables_equal_oracle_bit_for_bit (no other GPU test notices that change); `fabsf(a)` read as `a` fails it at the
70 x 66 scene and test_threshold_pairs_differ_where_the_model_says at `gate_par-`; without `|| dt2 > r2 * ds2` the
same two tests fail, the second at `ratio_t`; with mode 3's odometry block skipped they fail in mode 3; and without
estimate_pose's `det33(Rm) > 0` retry test_register_equals_oracle and
test_register_against_model_and_construction fail (0.88 rad off at the 33 x 31 scene)."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import _match_cases as Cs
import match_model as M
import rgbd360_amd as R
from oracle import oracle360 as O
from oracle import persist_oracle as PO

pytestmark = pytest.mark.gpu

ROT_BAR, TRANS_BAR = 1e-4, 1e-3        # rad, m: the north-star bar
INFO_BAR = 2.0 ** -22                  # relative; the float32 store of the float64 sums accounts for 2^-24
INI_PATH = {ini: (os.path.join(Cs.CONFIG_DIR, ini) if ini else None) for ini in Cs.INIS}


@pytest.fixture(scope="module")
def ctx():
    return R.Context(0)


@pytest.fixture(scope="module")
def cal(ctx):
    return R.Calib360(ctx, 48, 64)     # the frames hold loaded planes only; their image buffers stay unused


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (path of the map's file, payload) for every plane list, written once."""
    d = tmp_path_factory.mktemp("maps")
    seen = {}

    def path_of(planes, tag):
        if tag not in seen:
            p = str(d / f"m{len(seen)}.pbmap")
            seen[tag] = (p, PO.pbmap_write(p, planes))
        return seen[tag]
    return path_of


def _load(frame, files, case, ini, side):
    frame.loadPbMap(files(case[side], (case["name"], ini, side))[0])
    return frame


def _omaps(case):
    return O.PbMap.from_planes(case["ref"]), O.PbMap.from_planes(case["trg"])


_oracle = {}


def _oracle_tables(case, ini, mode):
    key = (case["name"], ini, mode)
    if key not in _oracle:
        a, b = _omaps(case)
        cap = max(len(case["ref"]), len(case["trg"]), 1)
        _oracle[key] = O.match_tables(a, b, case["mmp"], mode, cap=cap, params=Cs.params(ini))
    return _oracle[key]


def _gpu_tables(ctx, cal, files, cases):
    """Every case in order on one context: key -> the four tables' bytes."""
    f1, f2 = R.Frame360(cal), R.Frame360(cal)
    out = {}
    regs = {ini: R.RegisterRGBD360(ctx, INI_PATH[ini]) for ini in Cs.INIS}
    for case, ini, _ in cases:
        reg = regs[ini]
        reg.setReference(_load(f1, files, case, ini, "ref"), case["mmp"])
        reg.setTarget(_load(f2, files, case, ini, "trg"), case["mmp"])
        for mode in range(4):
            out[(case["name"], ini, mode)] = reg.match_tables(mode, cap=max(len(case["ref"]), len(case["trg"]), 1))
    return out


@pytest.fixture(scope="module")
def table_cases():
    return Cs.all_table_cases()


@pytest.fixture(scope="module")
def gpu_tables(ctx, cal, files, table_cases):
    return _gpu_tables(ctx, cal, files, table_cases)


def test_tables_equal_oracle_bit_for_bit(gpu_tables, table_cases):
    """Every case (70 x 66 first, then the small shapes on the context whose tables have grown), every mode, both
    threshold sets; the exact family and the NaN plane included.  Padding bits of each row's last word are zero."""
    n = 0
    for case, ini, _ in table_cases:
        for mode in range(4):
            g, o = gpu_tables[(case["name"], ini, mode)], _oracle_tables(case, ini, mode)
            tag = (case["name"], ini, mode)
            for key in ("sid", "tid", "unary", "binary"):
                assert np.array_equal(g[key], o[key]), tag + (key,)
            ns, nt = len(g["sid"]), len(g["tid"])
            assert g["words"] == (ns * nt + 63) // 64, tag
            if ns and nt:
                _, pad = M.unpack(g["binary"], ns, nt)
                assert not pad.any(), tag
            n += 1
    assert n == 4 * len(table_cases)


def test_tables_equal_the_model_where_it_decides(gpu_tables, table_cases):
    und = tot = 0
    first = {}
    for case, ini, _ in table_cases:
        for mode in range(4):
            m = M.tables(case["ref"], case["trg"], case["mmp"], mode, Cs.params(ini),
                         binary_of=first.get((case["name"], ini)))
            first.setdefault((case["name"], ini), m)
            assert M.agree(m, gpu_tables[(case["name"], ini, mode)]) == [], (case["name"], ini, mode)
            u, n = M.undecided(m)
            und, tot = und + u, tot + n
    print(f"\n[match shapes] {und} of {tot} entries undecided by the model ({100.0 * und / tot:.4f} %)")


def test_threshold_pairs_differ_where_the_model_says(gpu_tables):
    """The two maps of a threshold pair differ on the GPU in exactly the entries in which the model's differ (the
    CPU suite checks that those are the entries the comparison governs)."""
    for ini in Cs.INIS:
        for th in Cs.threshold_cases(ini):
            for mode in range(4):
                lo, hi = (gpu_tables[(th[s]["name"], ini, mode)] for s in ("below", "above"))
                mlo, mhi = (M.tables(th[s]["ref"], th[s]["trg"], 0, mode, Cs.params(ini)) for s in ("below", "above"))
                tag = (th["name"], ini, mode)
                assert np.array_equal(lo["unary"] != hi["unary"], mlo["unary"] != mhi["unary"]), tag
                assert np.array_equal(M.unpack(lo["binary"], 2, 2)[0] != M.unpack(hi["binary"], 2, 2)[0],
                                      mlo["ok"] != mhi["ok"]), tag
                if mode in th["modes"]:
                    e = th["entry"]
                    got = (lo["unary"] != hi["unary"])[e[1], e[2]] if e[0] == "unary" else \
                        (M.unpack(lo["binary"], 2, 2)[0] != M.unpack(hi["binary"], 2, 2)[0])[e[1:]]
                    assert got, tag


def test_fresh_context_gives_the_same_bytes(cal, files, table_cases, gpu_tables):
    """The same cases on a context that has served nothing before (its tables grow once, at the first case)."""
    ctx2 = R.Context(0)
    cal2 = R.Calib360(ctx2, 48, 64)
    again = _gpu_tables(ctx2, cal2, files, table_cases)
    assert again.keys() == gpu_tables.keys()
    for key, g in gpu_tables.items():
        for k in ("sid", "tid", "unary", "binary"):
            assert g[k].tobytes() == again[key][k].tobytes(), key + (k,)
    # and a small case first, the large one after, a small one again: growth in the middle of a context's life
    ctx3 = R.Context(0)
    cal3 = R.Calib360(ctx3, 48, 64)
    by_name = {c["name"]: (c, ini, x) for c, ini, x in table_cases if ini is None}
    order = [by_name[n] for n in ("scene3x3s105", "scene40x3s106", "scene70x66s100", "scene2x3s103", "scene64x2s104")]
    third = _gpu_tables(ctx3, cal3, files, order)
    for key, g in third.items():
        for k in ("sid", "tid", "unary", "binary"):
            assert g[k].tobytes() == gpu_tables[key][k].tobytes(), key + (k,)


# ------------------------------------------------------------------------------------------------ registration
def _register_cases():
    return Cs.shape_cases() + [Cs.twin_case()] + Cs.selection_cases() + Cs.pose_cases()


def test_register_equals_oracle(ctx, cal, files):
    """As test_gpu_planes.test_match_tables_and_register_pbmap asserts it: verdict, matches, matched area, areaSource /
    areaTarget, pose and information bit for bit, the tree not truncated."""
    f1, f2 = R.Frame360(cal), R.Frame360(cal)
    good = 0
    for ini in Cs.INIS:
        for case in _register_cases():
            _load(f1, files, case, ini, "ref"), _load(f2, files, case, ini, "trg")
            a, b = _omaps(case)
            for mode in case["modes"]:
                reg = R.RegisterRGBD360(ctx, INI_PATH[ini])
                calls0, trunc0, _ = ctx.match_stats()
                ok = reg.RegisterPbMap(f1, f2, case["mmp"], mode)
                calls1, trunc1, max_nodes = ctx.match_stats()
                r = O.register_pbmap(a, b, case["mmp"], mode, params=Cs.params(ini))
                tag = (case["name"], ini, mode)
                assert calls1 == calls0 + 1 and trunc1 == trunc0 and not r["truncated"] and max_nodes >= r["nodes"], tag
                assert ok == bool(r["good"]), tag
                assert reg.getMatchedPlanes() == r["matches"], tag
                assert reg.getAreaMatched() == r["area_matched"], tag
                if ok:
                    good += 1
                    assert np.array_equal(reg.getPose(), r["pose"]), tag
                    assert np.array_equal(reg.getInfoMat(), r["info"]), tag
                    assert reg.areaSource == r["area_src"] and reg.areaTarget == r["area_trg"], tag
    assert good > 0


def test_register_against_model_and_construction(ctx, cal, files):
    """Known answers: the matches are the construction's permutation, the pose is G and the model's pose within the
    north-star bar, the information the model's within 2^-22 relative; the mirrored map gives a proper rotation (the
    det <= 0 branch), equal to the model's determinant-corrected one."""
    f1, f2 = R.Frame360(cal), R.Frame360(cal)
    worst = dict(G=[0.0, 0.0], model=[0.0, 0.0], info=0.0)
    for case in Cs.shape_cases() + Cs.pose_cases():
        expect = case.get("expect", len(case["truth"]) >= 3)
        if expect not in (True, "proper"):
            continue
        _load(f1, files, case, None, "ref"), _load(f2, files, case, None, "trg")
        reg = R.RegisterRGBD360(ctx)
        assert reg.RegisterPbMap(f1, f2, case["mmp"], R.DEFAULT_6DoF), case["name"]
        assert reg.getMatchedPlanes() == case["truth"], case["name"]
        ok, P, info = M.pose(case["ref"], case["trg"], case["truth"])
        assert ok
        got = reg.getPose().astype(np.float64)
        dr, dt = M.pose_drift(got, P)
        worst["model"] = [max(worst["model"][0], dr), max(worst["model"][1], dt)]
        assert dr <= ROT_BAR and dt <= TRANS_BAR, (case["name"], dr, dt)
        rel = np.abs(reg.getInfoMat().astype(np.float64) - info).max() / np.abs(info).max()
        worst["info"] = max(worst["info"], rel)
        assert rel <= INFO_BAR, (case["name"], rel)
        if expect is True:
            dr, dt = M.pose_drift(got, case["G"])
            worst["G"] = [max(worst["G"][0], dr), max(worst["G"][1], dt)]
            assert dr <= ROT_BAR and dt <= TRANS_BAR, (case["name"], dr, dt)
        else:
            Rm = got[:3, :3]
            assert abs(np.linalg.det(Rm) - 1) < 1e-5 and np.abs(Rm.T @ Rm - np.eye(3)).max() < 1e-5   # float32 entries
    print(f"\n[match shapes] pose against G: {worst['G'][0]:.2e} rad {worst['G'][1]:.2e} m; against the model: "
          f"{worst['model'][0]:.2e} rad {worst['model'][1]:.2e} m; information: {worst['info']:.2e} relative")


def _raw_register(ctx, f1, f2, mmp, mode, fill):
    """r360_register_pbmap itself, with every output preset to `fill`: the façade keeps its own copies."""
    pose, info = np.full(16, fill, np.float32), np.full(36, fill, np.float32)
    pairs = np.zeros(512, np.int32)
    n, am, as_, at = C.c_int(), C.c_float(), C.c_float(fill), C.c_float(fill)
    m = R.MatchParams.default()
    assert R.lib().r360_ctx_set_match_params(ctx.h, C.byref(m)) == 0
    rc = R.lib().r360_register_pbmap(ctx.h, f1.h, f2.h, mmp, mode, R._fptr(pose), R._fptr(info),
                                     pairs.ctypes.data_as(C.POINTER(C.c_int)), 256, C.byref(n), C.byref(am),
                                     C.byref(as_), C.byref(at))
    return rc, pose, info, n.value, as_.value, at.value


def test_failed_call_leaves_pose_untouched(ctx, cal, files):
    """Fewer than three matches, a corridor, parallel normals, conditioning above 8000 and the NaN plane return 0 and
    write neither pose nor information nor the two map areas; the conditioning just below 8000 returns 1."""
    f1, f2 = R.Frame360(cal), R.Frame360(cal)
    by_name = {c["name"]: c for c in Cs.pose_cases()}
    fill = np.float32(-7.25)
    for name in ("two", "corridor", "parallel", "cond+", "nan"):
        case = by_name[name]
        _load(f1, files, case, None, "ref"), _load(f2, files, case, None, "trg")
        rc, pose, info, n, as_, at = _raw_register(ctx, f1, f2, 0, R.DEFAULT_6DoF, fill)
        assert rc == 0 and n == len(case["truth"]), (name, rc, n)
        assert (pose == fill).all() and (info == fill).all() and as_ == fill and at == fill, name
        if name == "nan":
            r = O.register_pbmap(*_omaps(case), 0, O.DEFAULT_6DoF)
            print(f"\n[match shapes] NaN plane: {n} matches, rc {rc}; oracle {len(r['matches'])} matches, good {r['good']}")
            assert r["good"] == rc and len(r["matches"]) == n
    case = by_name["cond-"]
    _load(f1, files, case, None, "ref"), _load(f2, files, case, None, "trg")
    rc, pose, info, n, as_, at = _raw_register(ctx, f1, f2, 0, R.DEFAULT_6DoF, fill)
    assert rc == 1 and n == 3 and not (pose == fill).any() and as_ != fill and at != fill


def test_batch_of_crafted_pairs_equals_lone_calls(ctx, cal, files):
    """16 PbMap jobs of mixed size, (3, 3) to (40, 3), over a 4-lane Batch: every job's result is the lone call's,
    twice."""
    want = {(3, 3), (40, 3), (7, 9), (3, 40), (8, 8), (25, 25), (5, 13), (13, 5)}
    cases = [c for c in Cs.shape_cases() if (len(c["ref"]), len(c["trg"])) in want]
    assert len(cases) == 8
    frames, lone = [], []
    for case in cases:
        f1, f2 = R.Frame360(cal), R.Frame360(cal)
        _load(f1, files, case, None, "ref"), _load(f2, files, case, None, "trg")
        frames.append((f1, f2))
        reg = R.RegisterRGBD360(ctx)
        ok = reg.RegisterPbMap(f1, f2, 0, R.DEFAULT_6DoF)
        lone.append((ok, reg))
    order = [0, 1, 2, 3, 4, 5, 6, 7, 5, 1, 0, 7, 3, 2, 6, 4]
    batch = R.Batch(0, lanes=4)
    for _ in range(2):
        res = batch.register_pairs([{"ref": frames[k][0], "trg": frames[k][1]} for k in order], 0, R.DEFAULT_6DoF)
        assert len(res) == 16
        for k, r in zip(order, res):
            ok, reg = lone[k]
            assert r["good"] == int(ok) and r["n_match"] == len(reg.getMatchedPlanes()), cases[k]["name"]
            assert r["area_matched"] == reg.getAreaMatched()
            if ok:
                assert r["pbmap_pose"].tobytes() == reg.getPose().tobytes(), cases[k]["name"]
                assert r["pbmap_info"].tobytes() == reg.getInfoMat().tobytes(), cases[k]["name"]
                assert r["area_src"] == reg.areaSource and r["area_trg"] == reg.areaTarget
    assert all(ok for ok, _ in lone)                # each of these pairs shares three or more planes
    batch.close()


# ------------------------------------------------------------------------------------------------ files
def test_save_load_save_reproduces_the_writer(cal, files, tmp_path):
    case = [c for c in Cs.shape_cases() if len(c["ref"]) == 25][0]
    nan = [c for c in Cs.pose_cases() if c["name"] == "nan"][0]
    for k, planes in enumerate((case["ref"], nan["trg"])):
        src, payload = files(planes, ("resave", k))
        f = R.Frame360(cal)
        f.loadPbMap(src)
        a, b = str(tmp_path / f"a{k}.pbmap"), str(tmp_path / f"b{k}.pbmap")
        f.savePlanes(a)
        assert gzip.open(a).read() == payload
        g = R.Frame360(cal)
        g.loadPbMap(a)
        g.savePlanes(b)
        assert gzip.open(b).read() == payload


def test_load_rejects_plane_ids_out_of_order(cal, files, tmp_path):
    """A file whose ids are not 0..n-1 in order would index the plane vector out of bounds in the matcher: loadPbMap
    refuses it and leaves the frame's planes and build flags as they were."""
    case = Cs.shape_cases()[5]                       # 3 x 3
    f = R.Frame360(cal)
    fresh = R.Frame360(cal)
    fresh_flags = fresh.built()
    f.loadPbMap(files(case["ref"], ("ids", 0))[0])
    before, flags = f.planes(), f.built()
    for k, ids in enumerate(((1, 0, 2), (0, 1, 7), (0, 0, 1), (-1, 0, 1))):
        bad = str(tmp_path / f"bad{k}.pbmap")
        PO.pbmap_write(bad, [dict(p, id=i) for p, i in zip(case["trg"], ids)])
        for frame in (f, fresh):
            with pytest.raises(RuntimeError, match="plane ids are not 0..n-1"):
                frame.loadPbMap(bad)
    after = f.planes()
    assert f.built() == flags and len(after) == len(before)
    for p, q in zip(before, after):
        assert np.array_equal(p["normal"], q["normal"]) and p["area"] == q["area"] and p["id"] == q["id"]
    assert fresh.built() == fresh_flags and not (fresh_flags & R.BUILD_PLANES)
    with pytest.raises(RuntimeError):
        fresh.planes()
