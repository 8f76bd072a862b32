"""The control-plane files through the library, without a GPU: the reference's correspondences_i_j.txt
(tests/golden/control_planes.npz, written out as text by _rigcal_cases.golden_dir) read and written by r360_rigcal_load_dir / _save_dir and the bare matrix codec."""
import os

import numpy as np
import pytest

import rgbd360_amd as R

import _rigcal_cases as Cs
import rigcal_model as M


@pytest.fixture()
def cal():
    c = R.RigCalibration(None)
    yield c
    c.close()


def test_fixture_directory_round_trips_byte_for_byte(cal, tmp_path):
    golden = Cs.golden_dir()
    # the directory written from the archive holds the reference's own bytes: every written file hashes to what the
    # reference's file hashed to when the archive was made
    import hashlib
    assert len(Cs.GOLDEN_SHA256) == 11
    for key, sha in Cs.GOLDEN_SHA256.items():
        data = open(os.path.join(golden, f"correspondences_{key}.txt"), "rb").read()
        assert hashlib.sha256(data).hexdigest() == sha, key
    cal.loadPlaneCorrespondences(golden)
    want = M.load_dir(golden)
    got = cal.pairs()
    assert sorted(got) == sorted(want) and len(want) == 11
    for p in want:
        assert np.array_equal(got[p], want[p]), p
    assert sum(len(got[p]) for p in Cs.ADJACENT) == 1090
    cal.savePlaneCorrespondences(str(tmp_path))
    names = sorted(os.listdir(tmp_path))
    assert names == sorted(f for f in os.listdir(golden) if f.endswith(".txt"))
    for f in names:
        assert (tmp_path / f).read_bytes() == open(os.path.join(golden, f), "rb").read(), f


def test_bare_matrix_codec(tmp_path):
    rng = np.random.default_rng(3)
    a = rng.normal(size=(7, 10)) * 10.0 ** rng.integers(-8, 8, size=(7, 10))
    path = str(tmp_path / "m.txt")
    R.rigcal_write_matrix(path, a)
    assert np.array_equal(R.rigcal_read_matrix(path), a)
    assert np.array_equal(np.loadtxt(path, ndmin=2), a)
    with open(path, "w") as f:
        f.write("% a comment\n1 2 3\n4 5\n")
    with pytest.raises(RuntimeError, match="ragged"):
        R.rigcal_read_matrix(path)
    with pytest.raises(RuntimeError):
        R.rigcal_read_matrix(path + ".missing")


def test_missing_adjacent_pair_is_an_error_code(cal):
    cal.loadPlaneCorrespondences(Cs.golden_dir())
    assert cal.check() == 0
    cal.setPair(3, 4, cal.getPair(3, 4)[:2])
    assert cal.check() == R.EMISSING_PAIR
    cal.setPair(3, 4, cal.getPair(3, 4)[:0])
    assert cal.check() == R.EMISSING_PAIR and (3, 4) not in cal.pairs()
    cal.clear()
    assert cal.pairs() == {} and cal.check() == R.EMISSING_PAIR


def test_pairs_and_columns_are_checked(cal):
    rows = np.ones((4, 10))
    for i, j in ((1, 1), (3, 2), (0, 8), (-1, 2)):
        with pytest.raises(RuntimeError):
            cal.setPair(i, j, rows)
    with pytest.raises(RuntimeError, match="10 columns"):
        R._check(R.lib().r360_rigcal_set_pair(cal.h, 0, 1, R._dptr(np.ones((4, 18))), 4, 18), "set_pair")
    bad = rows.copy()
    bad[2, 5] = np.nan
    with pytest.raises(RuntimeError):
        cal.setPair(0, 1, bad)


def test_specs_and_host_only_handle(cal, tmp_path):
    S = R.rigcal_specs()
    assert np.abs(S - M.construction_specs()).max() <= 1e-15
    assert S[0][2, 3] == 0.055 and np.array_equal(cal.estimate(), S)
    rig = Cs.perturbed_rig(2)
    cal.setInit(rig)
    assert np.array_equal(cal.estimate(), rig)
    with pytest.raises(RuntimeError, match="without a context"):
        cal.CalibrateRotation()
    # Rt_0k.txt as r360_calib_load_extrinsics reads them: row-major text, float precision
    cal.saveExtrinsics(str(tmp_path))
    for k in range(8):
        T = np.loadtxt(tmp_path / f"Rt_0{k + 1}.txt")
        assert np.array_equal(T.astype(np.float32), rig[k].astype(np.float32))


def test_calibrator_call_sites_compile_unchanged(root):
    """Source-level drop-in of Calibration/Calibrator.cpp:64-75, 176-192 (tests/dropin/calibrator_dropin.cpp) and the
    CalibrateRig driver, against the façade with g++ alone."""
    import subprocess
    for src in ("tests/dropin/calibrator_dropin.cpp", "apps/CalibrateRig.cpp"):
        p = subprocess.run(["g++", "-std=c++17", "-O0", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", f"-I{root}/include",
                            f"{root}/{src}"], capture_output=True, text=True)
        assert p.returncode == 0, (src, p.stderr[-3000:])
