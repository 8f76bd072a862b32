"""The numpy statement of the rig calibration (tests/rigcal_model.py) on synthetic rigs and on the reference's shipped
control planes (tests/golden/control_planes.npz).

Without noise the translation system is linear and Gauss-Newton is exact at a zero residual, so the model recovers the
rig: relative rotations to 1e-9 rad, relative translations to 1e-9 m.  CalibrateRotation's own stop constants (1e-5
on |update|^2) end one call near 1e-8 rad, one quadratic step short; a second call started from the first's estimate
reaches the bar, and that is what is asserted.  The fixture figures are the model's regression values."""
import numpy as np
import pytest

import _rigcal_cases as Cs
import rigcal_model as M


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_recovers_a_noise_free_rig(seed):
    rig = Cs.perturbed_rig(seed)
    rows = Cs.make_rows(rig, {p: 20 for p in Cs.ADJACENT}, seed + 10)
    Rt, st = M.calibrate_rotation(rows, M.construction_specs())
    assert st["status"] == M.STATUS_CONVERGED
    dr1, _ = Cs.relative_errors(Rt, rig)
    Rt, st = M.calibrate_rotation(rows, Rt)
    assert st["status"] == M.STATUS_CONVERGED
    Rt, st = M.calibrate_translation(rows, Rt)
    assert st["status"] == M.STATUS_CONVERGED
    dr, dt = Cs.relative_errors(Rt, rig)
    print(f"seed {seed}: first call {dr1:.2e} rad; restarted {dr:.2e} rad, {dt:.2e} m")
    assert dr1 < 1e-6
    assert dr <= 1e-9 and dt <= 1e-9
    # the recentring (:1311-1320): t_0 = -(sum of the seven updates) / 8
    upd = [Rt[k][:3, 3] - Rt[0][:3, 3] for k in range(1, 8)]
    assert np.allclose(Rt[0][:3, 3], -np.sum(upd, axis=0) / 8, atol=1e-15)


def test_all_pairs_and_weights_recover_the_rig_too():
    rig = Cs.perturbed_rig(4)
    rows = Cs.make_rows(rig, {p: 6 for p in M.PAIRS}, 14)
    for weighted in (False, True):
        Rt, _ = M.calibrate_rotation(rows, M.construction_specs(), weighted)
        Rt, _ = M.calibrate_rotation(rows, Rt, weighted)
        Rt, st = M.calibrate_translation(rows, Rt, weighted)
        dr, dt = Cs.relative_errors(Rt, rig)
        print(f"weighted {weighted}: {dr:.2e} rad, {dt:.2e} m")
        assert st["status"] == M.STATUS_CONVERGED and dr <= 1e-9 and dt <= 1e-9


def test_block_pattern_keeps_the_reference_quirks():
    """Sensor 0's rows and cross block are skipped; the lower cross block is the transpose of the upper."""
    rig = Cs.perturbed_rig(5)
    rows = Cs.make_rows(rig, Cs.base_counts({(0, 7): 5, (0, 3): 4, (2, 5): 7}), 15, noise=1e-2)
    H, g, sc = M.accumulate(rows, M.construction_specs(), M.MODE_ROTATION, False)
    blk = lambda a, b: H[3 * a - 3:3 * a, 3 * b - 3:3 * b]
    assert sc[2] == 7 * 3 + 5 + 4 + 7
    assert np.any(blk(2, 5)) and np.array_equal(blk(5, 2), blk(2, 5).T)
    assert not np.any(blk(3, 7)) and not np.any(blk(1, 3))      # (0, 3) and (0, 7) leave no cross block
    assert np.any(blk(1, 2)) and not np.any(blk(1, 4))
    assert np.array_equal(H, H.T)


def test_missing_pair_and_bad_conditioning():
    rig = Cs.perturbed_rig(6)
    counts = Cs.base_counts({(0, 7): 5})
    counts[(3, 4)] = 2
    S = M.construction_specs()
    Rt, st = M.calibrate_rotation(Cs.make_rows(rig, counts, 16), S)
    assert st["status"] == M.STATUS_MISSING_PAIR and np.array_equal(Rt, S)
    rows = Cs.make_rows(rig, Cs.base_counts(n=5), 17, parallel=[0.6, 0.0, 0.8])
    Rt, st = M.calibrate_rotation(rows, S)
    assert st["status"] == M.STATUS_BAD_CONDITIONED and len(st["iterations"]) == 1
    assert np.array_equal(Rt, S)                                 # the alignment's system is singular at the specs
    Rt2, st = M.calibrate_translation(rows, Rt)
    assert st["status"] == M.STATUS_BAD_CONDITIONED and np.array_equal(Rt2, Rt)


def test_vertical_alignment_turns_the_mean_x_axis_up():
    Rt = Cs.perturbed_rig(7)
    out = M.vertical_alignment(Rt)
    mean = lambda P: np.mean([T[:3, 0] for T in P], axis=0)
    a, b = mean(Rt), mean(out)
    print("mean X axis", a, "->", b)
    assert np.hypot(b[1], b[2]) < 0.05 * np.hypot(a[1], a[2])
    for k in range(1, 8):                                        # a common turn: the relative rotations stay
        assert np.allclose(Rt[0][:3, :3].T @ Rt[k][:3, :3], out[0][:3, :3].T @ out[k][:3, :3], atol=1e-14)


def test_fixture_regression_adjacent():
    """Adjacent_Int: 1,090 rows, three iterations, the third step rejected."""
    rows = Cs.fixture_rows()
    Rt, st = M.calibrate_rotation(rows, M.construction_specs())
    it = st["iterations"]
    assert st["rows"] == 1090 and st["status"] == M.STATUS_CONVERGED and len(it) == 3
    assert [r["accepted"] for r in it] == [True, True, False]
    dec = [r["werr0"] - r["werr1"] for r in it]
    print("decreases", dec, "cond", [r["cond"] for r in it])
    assert dec[0] == pytest.approx(17.714, abs=1e-3) and dec[1] == pytest.approx(0.08665, abs=1e-5)
    assert dec[2] == pytest.approx(-3.008e-5, abs=1e-8)
    assert np.degrees(it[0]["angle"] / 1090) == pytest.approx(2.3753, abs=1e-4)
    assert np.degrees(it[1]["angle"] / 1090) == pytest.approx(1.9532, abs=1e-4)
    # the angle the reference prints (ErrorCalibRotation, :1217) is the last linearisation's, the third here
    assert np.degrees(it[2]["angle"] / 1090) == pytest.approx(1.9515, abs=1e-4)
    assert it[0]["cond"] == pytest.approx(55.504, abs=1e-3) and it[2]["cond"] == pytest.approx(55.874, abs=1e-3)
    _, st = M.calibrate_translation(rows, Rt)
    assert st["status"] == M.STATUS_CONVERGED and st["cond"] == pytest.approx(148.001, abs=1e-3)


def test_draw_gives_three_distinct_rows():
    for n in (3, 4, 5, 64, 1000):
        seen = set()
        for trial in range(200):
            idx = M.draw3(9, trial, trial % 7, n)
            assert len(set(idx)) == 3 and all(0 <= i < n for i in idx)
            seen.update(idx)
        assert seen == set(range(n)) if n <= 64 else len(seen) > 400


def test_trimmer_on_the_fixture_and_on_planted_outliers():
    fx = Cs.fixture_rows()
    for pair, n, best in (((0, 7), 178, 172), ((4, 5), 104, 102)):
        res = [M.score_trial(fx[pair], 7, t) for t in range(512)]
        flagged = sum(r[3] for r in res)
        print(pair, "best of 512 trials", max(r[0] for r in res), "flagged", flagged)
        assert len(fx[pair]) == n and max(r[0] for r in res) == best and flagged <= 5
    rig = Cs.perturbed_rig(5)
    rows = Cs.make_rows(rig, {(2, 3): 300}, 340, noise=1e-3)[(2, 3)]
    dirty, planted = Cs.with_outliers(rows, 0.2, 300)
    kept, st = M.trim(dirty, 7)
    print("300 rows, 60 planted:", st["inliers"], "kept after", st["trials"], "trials, winner", st["winner"])
    assert not st["no_model"] and not np.any(st["mask"] & planted) and st["inliers"] >= 230
    assert np.array_equal(kept, dirty[st["mask"]])


def test_trimmer_leaves_small_and_degenerate_sets_untouched():
    rig = Cs.perturbed_rig(5)
    rows = Cs.make_rows(rig, {(2, 3): 3}, 3)[(2, 3)]
    kept, st = M.trim(rows, 1)
    assert kept is rows and st["trials"] == 0 and not st["no_model"]
    rows = Cs.make_rows(rig, {(2, 3): 12}, 4, parallel=[0.0, 0.6, 0.8])[(2, 3)]
    kept, st = M.trim(rows, 1, max_iter=50)
    assert kept is rows and st["no_model"] and st["trials"] == 50 and st["winner"] == -1
