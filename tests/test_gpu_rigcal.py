"""Rig extrinsic calibration on the GPU (kernels/rigcal_kernels.hip, host/rigcal.cpp) against its numpy statement
tests/rigcal_model.py, on the reference's control planes (tests/golden/control_planes.npz) and the synthetic rigs of
tests/_rigcal_cases.py.

Bars.  One linearisation: H within 1e-12 of max |H|, g within 1e-12 of max |g|, the scalars within 1e-12 relative and
the zero / non-zero pattern of H equal -- both sides add the same fp64 terms and only the grouping differs.  A whole
solve: status, iteration count and every accept decision equal, the per-iteration error and conditioning within 1e-9
relative, every estimated pose within 1e-9 rad and 1e-9 m.  Two figures are not measured relative to themselves, for
a stated reason: the trial error werr1 is only ever used in werr1 < werr0 and werr0 - werr1 > 1e-6, so it is held to
1e-9 of werr0 (at a noise-free rig it is 1e-32, rounding noise with no relative meaning), and |update|^2 is only ever
compared with 1e-5, so it is held to 1e-9 of max(|update|^2, 1e-5).  The trimmer: per-trial inlier count and no-draw flag
equal, except on trials the model flags as having a row within 1e-9 of a threshold (at most 1 % of the trials); the
winner, the trials run and the mask equal to the model's sequential run at every chunk size.  The collector: rows
equal to the model's collector fed with the frame's local planes and label image, columns 0-7 within 1e-12 (the same
floats go into both), columns 8-9 exactly (integers and one division).  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import rgbd360_amd as R

import _rigcal_cases as Cs
import rigcal_model as M

pytestmark = pytest.mark.gpu

SEED = 7


@pytest.fixture(scope="module")
def ctx():
    c = R.Context(0)
    yield c
    c.close()


_OPEN = []


@pytest.fixture(autouse=True)
def _close_handles():
    yield
    while _OPEN:
        _OPEN.pop().close()


def _new(ctx, rows=None, init=None):
    c = R.RigCalibration(ctx)
    _OPEN.append(c)
    if rows is not None:
        c.setPairs(rows)
    if init is not None:
        c.setInit(init)
    return c


ALL_28 = {p: 3 + (5 * k) % 11 for k, p in enumerate(M.PAIRS)}
EVAL_CASES = {
    "one_row": Cs.base_counts({(2, 5): 1}),
    "wave_edge": Cs.base_counts({(1, 3): 63, (2, 4): 64, (3, 6): 65}),
    "workgroup_edge": Cs.base_counts({(1, 4): 255, (2, 6): 256, (3, 7): 257, (4, 5): 513}),
    "adjacent_only": Cs.base_counts(),
    "adjacent_and_07": Cs.base_counts({(0, 7): 9}),
    "all_28": ALL_28,
    "sensor_0_extras": Cs.base_counts({(0, 2): 5, (0, 3): 70, (0, 5): 4, (0, 7): 300}),
}


@pytest.mark.parametrize("name", sorted(EVAL_CASES))
def test_eval_parity(ctx, name):
    truth = Cs.perturbed_rig(21)
    rows = Cs.make_rows(truth, EVAL_CASES[name], 31, noise=1e-2)
    cal = _new(ctx, rows)
    for where, Rt in (("specs", M.construction_specs()), ("perturbed", Cs.perturbed_rig(22))):
        cal.setInit(Rt)
        for mode in (M.MODE_ROTATION, M.MODE_TRANSLATION):
            for weighted in (False, True):
                H, g, sc = cal.eval(mode, weighted)
                mH, mg, msc = M.accumulate(rows, Rt, mode, weighted)
                eH = np.abs(H - mH).max() / np.abs(mH).max()
                eg = np.abs(g - mg).max() / np.abs(mg).max()
                es = max(abs(a - b) / abs(b) if b else abs(a) for a, b in zip(sc, msc))
                print(f"{name} {where} mode {mode} weighted {int(weighted)}: H {eH:.2e} g {eg:.2e} scalars {es:.2e} rows {sc[2]:.0f}")
                assert eH <= 1e-12 and eg <= 1e-12 and es <= 1e-12
                assert sc[2] == msc[2]
                assert np.array_equal(H == 0.0, mH == 0.0)


def test_missing_pair_status(ctx):
    counts = Cs.base_counts({(0, 7): 5})
    counts[(4, 5)] = 2
    rows = Cs.make_rows(Cs.perturbed_rig(21), counts, 32, noise=1e-2)
    cal = _new(ctx, rows)
    assert cal.eval(0) == R.EMISSING_PAIR
    st = cal.CalibrateRotation()
    assert st.status == R.RIGCAL_MISSING_PAIR and st.iterations == 0
    assert np.array_equal(cal.estimate(), R.rigcal_specs())
    assert cal.CalibrateTranslation().status == R.RIGCAL_MISSING_PAIR


def _compare_solve(tag, cal, rows, init, weighted):
    mRt, mst = M.calibrate_rotation(rows, init, weighted)
    cal.setInit(init)
    st = cal.CalibrateRotation(weighted)
    n = len(mst["iterations"])
    print(f"{tag}: status {st.status}/{mst['status']} iterations {st.iterations}/{n} rows {st.rows}")
    assert st.status == mst["status"] and st.iterations == n
    for k, r in enumerate(mst["iterations"]):
        rel = lambda a, b: abs(a - b) / abs(b)
        # the trial error is only ever compared with the error before the step, so it is measured on that scale
        figs = (rel(st.error[k], r["error"]), rel(st.angle[k], r["angle"]), rel(st.conditioning[k], r["cond"]),
                rel(st.werr0[k], r["werr0"]), abs(st.werr1[k] - r["werr1"]) / abs(r["werr0"]), abs(st.update2[k] - r["update2"]))
        print(f"  it {k}: error {st.error[k]:.6g} cond {st.conditioning[k]:.6g} accepted {st.accepted[k]}/{int(r['accepted'])} "
              f"decrease {st.werr0[k] - st.werr1[k]:.3e}; rel diffs {['%.1e' % f for f in figs]}")
        assert bool(st.accepted[k]) == r["accepted"]
        assert max(figs[:5]) <= 1e-9 and figs[5] <= 1e-9 * max(r["update2"], M.EPSILON_TRANSF)
    dr, dt = Cs.pose_diff(cal.estimate(), mRt)
    print(f"  rotation estimate: {dr:.2e} rad {dt:.2e} m")
    assert dr <= 1e-9 and dt <= 1e-9
    mRt2, mst2 = M.calibrate_translation(rows, mRt, weighted)
    st2 = cal.CalibrateTranslation(weighted)
    dr, dt = Cs.pose_diff(cal.estimate(), mRt2)
    print(f"  translation: status {st2.status}/{mst2['status']} cond {st2.conditioning[0]:.6g}/{mst2['cond']:.6g} "
          f"error {st2.error[0]:.6g}; estimate {dr:.2e} rad {dt:.2e} m")
    assert st2.status == mst2["status"] and st2.rows == mst2["rows"]
    assert abs(st2.conditioning[0] - mst2["cond"]) <= 1e-9 * mst2["cond"] and abs(st2.error[0] - mst2["error"]) <= 1e-9 * mst2["error"]
    assert dr <= 1e-9 and dt <= 1e-9
    return cal.estimate()


@pytest.mark.parametrize("adjacent_only", [True, False])
def test_whole_solve_on_the_fixture(ctx, adjacent_only):
    rows = Cs.fixture_rows(adjacent_only)
    cal = _new(ctx, rows)
    for weighted in (False, True):
        _compare_solve(f"fixture adjacent_only={adjacent_only} weighted={weighted}", cal, rows, M.construction_specs(), weighted)


def test_whole_solve_on_synthetic_rigs(ctx):
    truth = Cs.perturbed_rig(1)
    rows = Cs.make_rows(truth, {p: 20 for p in Cs.ADJACENT}, 11)
    cal = _new(ctx, rows)
    est = _compare_solve("noise-free", cal, rows, M.construction_specs(), False)
    est = _compare_solve("noise-free, restarted", cal, rows, est, False)
    dr, dt = Cs.relative_errors(est, truth)
    print(f"against the true rig: {dr:.2e} rad {dt:.2e} m")
    assert dr <= 1e-9 and dt <= 1e-9
    rows = Cs.make_rows(Cs.perturbed_rig(2), ALL_28, 12, noise=5e-3)
    _compare_solve("noisy, all pairs, weighted", _new(ctx, rows), rows, M.construction_specs(), True)


def test_parallel_normals_are_bad_conditioned(ctx):
    rows = Cs.make_rows(Cs.perturbed_rig(6), Cs.base_counts(n=5), 17, parallel=[0.6, 0.0, 0.8])
    S = M.construction_specs()
    cal = _new(ctx, rows, S)
    st = cal.CalibrateRotation()
    print("rotation status", st.status, "conditioning", st.conditioning[0])
    assert st.status == R.RIGCAL_BAD_CONDITIONED and st.iterations == 1 and st.conditioning[0] > 8000
    mRt, _ = M.calibrate_rotation(rows, S)
    assert np.array_equal(cal.estimate(), mRt) and np.array_equal(mRt, S)
    st = cal.CalibrateTranslation()
    print("translation status", st.status, "conditioning", st.conditioning[0])
    assert st.status == R.RIGCAL_BAD_CONDITIONED and not st.accepted[0]
    assert np.array_equal(cal.estimate(), S)


def test_two_runs_give_identical_bytes(ctx):
    rows = Cs.fixture_rows(False)
    out = []
    for _ in range(2):
        cal = _new(ctx, rows)
        a = cal.CalibrateRotation(True)
        b = cal.CalibrateTranslation(True)
        H, g, sc = cal.eval(0, True)
        out.append(bytes(a) + bytes(b) + cal.estimate().tobytes() + H.tobytes() + g.tobytes() + sc.tobytes())
    assert out[0] == out[1]


def _trim_inputs():
    fx = Cs.fixture_rows()
    rig = Cs.perturbed_rig(5)
    inputs = {"fixture_0_7": ((0, 7), fx[(0, 7)], None), "fixture_4_5": ((4, 5), fx[(4, 5)], None)}
    for n in (4, 65, 300):
        rows = Cs.make_rows(rig, {(2, 3): n}, 40 + n, noise=1e-3)[(2, 3)]
        inputs[f"synthetic_{n}"] = ((2, 3),) + Cs.with_outliers(rows, 0.2, n)
    return inputs


TRIM_INPUTS = _trim_inputs()


@pytest.mark.parametrize("name", sorted(TRIM_INPUTS))
def test_ransac_trials_match_the_model(ctx, name):
    (i, j), rows, _ = TRIM_INPUTS[name]
    cal = _new(ctx, {(i, j): rows})
    counts, flags = cal.ransacEval(i, j, SEED, 0, 512)
    model = [M.score_trial(rows, SEED, t) for t in range(512)]
    near = np.array([m[3] for m in model])
    mc = np.array([m[0] for m in model])
    mf = np.array([0 if m[1] else 1 for m in model])
    differ = np.flatnonzero((counts != mc) | (flags != mf))
    print(f"{name}: {len(rows)} rows, best {counts.max()}/{mc.max()}, no-draw trials {flags.sum()}/{mf.sum()}, "
          f"flagged by the model {near.sum()}, differing {differ[:10]}")
    assert near.sum() <= 5                                   # 1 % of 512
    assert np.all(near[differ])
    # a second range starts where it says: the hash depends on the trial index alone
    c2, f2 = cal.ransacEval(i, j, SEED, 500, 12)
    assert np.array_equal(c2, counts[500:]) and np.array_equal(f2, flags[500:])


@pytest.mark.parametrize("name", sorted(TRIM_INPUTS))
def test_trim_matches_the_sequential_model_at_every_chunk_size(ctx, name):
    (i, j), rows, planted = TRIM_INPUTS[name]
    kept, mst = M.trim(rows, SEED)
    for chunk in (1, 64, 512, 0):
        cal = _new(ctx, {(i, j): rows})
        st, mask = cal.trimOutliersRANSAC(i, j, SEED, R.RigcalTrimParams.default(chunk=chunk))
        print(f"{name} chunk {chunk}: inliers {st.inliers}/{mst['inliers']} trials {st.trials}/{mst['trials']} "
              f"winner {st.winner}/{mst['winner']}")
        assert (st.inliers, st.trials, st.winner, st.no_model) == (mst["inliers"], mst["trials"], mst["winner"], 0)
        assert np.array_equal(mask, mst["mask"]) and np.array_equal(cal.getPair(i, j), kept)
    if name == "synthetic_300":
        assert planted.sum() == 60 and not np.any(mst["mask"] & planted)


def test_trim_leaves_small_and_degenerate_sets_untouched(ctx):
    rig = Cs.perturbed_rig(5)
    rows = Cs.make_rows(rig, {(2, 3): 3}, 3)[(2, 3)]
    cal = _new(ctx, {(2, 3): rows})
    st, mask = cal.trimOutliersRANSAC(2, 3, 1)
    assert (st.inliers, st.trials, st.winner, st.no_model) == (3, 0, -1, 0) and mask.all()
    assert np.array_equal(cal.getPair(2, 3), rows)
    rows = Cs.make_rows(rig, {(2, 3): 12}, 4, parallel=[0.0, 0.6, 0.8])[(2, 3)]
    cal = _new(ctx, {(2, 3): rows})
    prm = R.RigcalTrimParams.default(max_iterations=50, chunk=16)
    counts, flags = cal.ransacEval(2, 3, 1, 0, 50, prm)
    assert flags.all() and not counts.any()
    st, mask = cal.trimOutliersRANSAC(2, 3, 1, prm)
    _, mst = M.trim(rows, 1, max_iter=50)
    print("parallel normals: trials", st.trials, "no_model", st.no_model)
    assert mst["no_model"] and (st.inliers, st.trials, st.winner, st.no_model) == (12, 50, -1, 1) and mask.all()
    assert np.array_equal(cal.getPair(2, 3), rows)


def test_calibrate_rig_app_writes_loadable_extrinsics(ctx, tmp_path):
    """apps/CalibrateRig solve on the fixture directory (one child process): the reference's Error* lines, and eight
    Rt_0k.txt that r360_calib_load_extrinsics loads and that equal the library call's result in float."""
    import os
    import re
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "bin", "CalibrateRig")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build()"
    p = subprocess.run([exe, "solve", Cs.golden_dir(), str(tmp_path)], capture_output=True, text=True, timeout=100)
    assert p.returncode == 0, p.stderr + p.stdout[-2000:]
    print(p.stdout[-1500:])
    assert "1274 correspondences" in p.stdout
    m = re.search(r"ErrorCalibRotation (\S+) (\S+)", p.stdout)
    t = re.search(r"ErrorCalibTranslation (\S+)", p.stdout)
    assert m and t, p.stdout
    cal = _new(ctx)
    cal.loadPlaneCorrespondences(Cs.golden_dir())
    rs, ts = cal.Calibrate()
    assert float(m.group(1)) == pytest.approx(rs.werr0[rs.iterations - 1] / rs.rows, rel=1e-5)
    assert float(m.group(2)) == pytest.approx(rs.angle[rs.iterations - 1] / rs.rows, rel=1e-5)
    assert float(t.group(1)) == pytest.approx(ts.error[0] / ts.rows, rel=1e-5)
    want = cal.estimate().astype(np.float32)
    c360 = R.Calib360(ctx, 240, 320)
    c360.loadExtrinsicCalibration(str(tmp_path))
    rt = c360.extrinsics()[0]
    got = np.asarray(rt, np.float32).reshape(8, 4, 4).transpose(0, 2, 1)
    print("largest difference between the app's files and the library's estimate:", np.abs(got - want).max())
    assert np.array_equal(got, want)


def test_calibrate_rig_app_trims_like_the_library(ctx, tmp_path):
    """CalibrateRig solve --trim: ControlPlanes::trimOutliersRANSAC on every pair (seed 0), then the same solve."""
    import os
    import re
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "bin", "CalibrateRig")
    p = subprocess.run([exe, "solve", Cs.golden_dir(), str(tmp_path), "--trim"], capture_output=True, text=True, timeout=100)
    assert p.returncode == 0, p.stderr + p.stdout[-2000:]
    kept = {(int(a), int(b)): (int(c), int(d)) for a, b, c, d in re.findall(r"pair (\d) (\d): (\d+) of (\d+) rows kept", p.stdout)}
    cal = _new(ctx)
    cal.loadPlaneCorrespondences(Cs.golden_dir())
    rows = cal.pairs()
    for (i, j), r in rows.items():
        st, _ = cal.trimOutliersRANSAC(i, j, 0)
        _, mst = M.trim(r, 0)
        print((i, j), "kept", st.inliers, "of", len(r), "model", mst["inliers"], "app", kept.get((i, j)))
        assert kept[(i, j)] == (st.inliers, len(r)) and st.inliers == mst["inliers"]
    cal.Calibrate()
    want = cal.estimate().astype(np.float32)
    got = np.stack([np.loadtxt(tmp_path / f"Rt_0{k + 1}.txt") for k in range(8)]).astype(np.float32)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ the collector
COLLECT_FRAMES = 6
COLLECT_MIN_INLIERS = 1000     # the reference's; at 240x320 the plane stage sees 120x160 pixels per sensor


def _plane_bytes(f):
    n = R.C.c_int()
    R._check(R.lib().r360_frame_get_planes(f.h, None, 0, R.C.byref(n)), "get_planes")
    arr = (R.Plane * max(n.value, 1))()
    R._check(R.lib().r360_frame_get_planes(f.h, arr, n.value, R.C.byref(n)), "get_planes")
    return n.value, bytes(arr)[:n.value * R.C.sizeof(R.Plane)]


def test_collector_matches_the_model_and_its_rows_calibrate(ctx):
    """GetControlPlanes' loop on six synthetic frames of a rig whose true extrinsics are the specs perturbed by 2 deg /
    2 cm, built with the specs: the collected rows equal the model's collector fed with r360_frame_get_local_planes and
    the label image (columns 0-7 to 1e-12, 8-9 exactly), a build without the flag refuses and leaves the ordinary planes
    byte-equal, and the solve on the rows equals the model's and moves the rig towards the truth."""
    seed = 360 << 16
    specs = M.construction_specs()
    truth = Cs.perturbed_rig(77, deg=(2.0, 2.0), cm=(2.0, 2.0))
    c360 = R.Calib360(ctx, 240, 320)
    c360.setRt(specs)
    rt_built = np.asarray(c360.extrinsics()[0], np.float32).reshape(8, 4, 4).transpose(0, 2, 1).astype(np.float64)
    cal = _new(ctx)
    prm = R.RigcalCollectParams.default(min_inliers=COLLECT_MIN_INLIERS)
    want, cov = {}, np.zeros((8, 3, 3))
    base = R.synth_path_pose(seed, 0).astype(np.float64)
    for k in range(COLLECT_FRAMES):
        a = np.radians(60.0 * k)
        turn = np.eye(4)
        turn[1:3, 1:3] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]      # about the rig's vertical (X)
        bgr, dep = R.synth_frame_rt(240, 320, truth.astype(np.float32), seed, (base @ turn).astype(np.float32))
        f = R.Frame360(c360)
        f.upload(bgr, dep)
        f.build(R.BUILD_UNDISTORT | R.BUILD_PLANES | R.BUILD_LOCAL_PLANES)
        added = cal.addFrame(f, prm)
        local = [f.localPlanes(s) for s in range(8)]
        rows, c = M.collect(local, f.labels()[1], rt_built, min_inliers=COLLECT_MIN_INLIERS)
        cov += c
        for p, r in rows.items():
            want[p] = np.vstack([want[p], r]) if p in want else r
        print(f"frame {k}: local planes {[len(x) for x in local]}, rows added {int(added.sum())} (model {sum(len(r) for r in rows.values())})")
        assert [int(added[i]) for i in range(28)] == [len(rows.get(p, [])) for p in M.PAIRS]
        if k == 0:
            n1, b1 = _plane_bytes(f)
            g = R.Frame360(c360)
            g.upload(bgr, dep)
            g.build(R.BUILD_UNDISTORT | R.BUILD_PLANES)
            n0, b0 = _plane_bytes(g)
            assert n0 == n1 and n0 > 0 and b0 == b1
            with pytest.raises(RuntimeError, match="R360_BUILD_LOCAL_PLANES"):
                g.localPlanes(0)
            with pytest.raises(RuntimeError, match="R360_BUILD_LOCAL_PLANES"):
                cal.addFrame(g, prm)
            g.close()
        f.close()
    got = cal.pairs()
    print("rows per pair", {p: len(r) for p, r in got.items()})
    assert sorted(got) == sorted(want)
    for p in want:
        assert got[p].shape == want[p].shape
        d = np.abs(got[p][:, :8] - want[p][:, :8]).max()
        assert d <= 1e-12 and np.array_equal(got[p][:, 8:], want[p][:, 8:]), (p, d)
    cond, mcond = cal.conditioning(), M.adjacent_conditioning(cov)
    print("adjacent conditioning", cond, "model", mcond)
    assert np.allclose(cond, mcond, rtol=1e-6)          # the library returns floats (6e-8); numpy's sigma_min is good to 1e-9 here
    assert not M.missing_pair(want)
    est = _compare_solve("collected rows", cal, want, specs, False)
    before, _ = Cs.relative_errors(specs, truth)
    after, _ = Cs.relative_errors(est, truth)

    def mean_err(P):   # the mean over k of the angle between R_0^T R_k and the true rig's
        rel = lambda Q, k: Q[0][:3, :3].T @ Q[k][:3, :3]
        ang = lambda E: np.arccos(np.clip((np.trace(E) - 1.0) / 2.0, -1.0, 1.0))
        return np.degrees(np.mean([ang(rel(P, k).T @ rel(truth, k)) for k in range(1, 8)]))
    print(f"mean relative-rotation error against the true rig: specs {mean_err(specs):.3f} deg -> estimate {mean_err(est):.3f} deg")
    assert mean_err(est) < mean_err(specs)
    print(f"largest relative-rotation error against the true rig: specs {np.degrees(before):.3f} deg -> estimate {np.degrees(after):.3f} deg")
    assert after < before


def test_calibrate_rig_app_collects_like_the_library(ctx, tmp_path):
    """apps/CalibrateRig collect on three synthetic captures (one child process): the correspondences_i_j.txt it
    writes equal what the library collects from the same files with the same calibration."""
    import os
    import subprocess
    from oracle import oracle360 as O
    seed = 360 << 16
    truth = Cs.perturbed_rig(77, deg=(2.0, 2.0), cm=(2.0, 2.0)).astype(np.float32)
    for k in range(3):
        bgr, dep = R.synth_frame_rt(240, 320, truth, seed, R.synth_path_pose(seed, 4 * k))
        O.write_bin(str(tmp_path / f"sphere_images_{k + 1}.bin"), bgr, dep)
    out = tmp_path / "out"
    out.mkdir()
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "bin", "CalibrateRig")
    p = subprocess.run([exe, "collect", str(tmp_path), "1", str(out)], capture_output=True, text=True, timeout=100)
    assert p.returncode == 0, p.stderr + p.stdout[-2000:]
    print(p.stdout[-600:])
    c360 = R.Calib360(ctx, 240, 320)
    c360.loadIntrinsicCalibration(R.INTRINSICS_DIR)
    c360.setRt(M.construction_specs())
    cal = _new(ctx)
    for k in range(3):
        f = R.Frame360(c360)
        f.loadFrame(str(tmp_path / f"sphere_images_{k + 1}.bin"))
        f.build(R.BUILD_UNDISTORT | R.BUILD_PLANES | R.BUILD_LOCAL_PLANES)
        cal.addFrame(f)
        f.close()
    want, got = cal.pairs(), M.load_dir(str(out))
    assert "3 frames" in p.stdout and sum(len(r) for r in want.values()) > 20
    assert sorted(got) == sorted(want) and all(np.array_equal(got[q], want[q]) for q in want)
