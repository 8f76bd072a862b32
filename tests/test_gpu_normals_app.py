"""The normal estimation through the C++ façade: the PCL-shaped call sequence (tests/dropin/normals_dropin.cpp) and
KFsphereSLAM --map-normals / --save-map."""
import os
import re
import subprocess

import numpy as np
import pytest

import rgbd360_amd as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")


def test_dropin_runs(tmp_path):
    exe = os.path.join(BIN, "normals_dropin")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build()"
    p = subprocess.run([exe, str(tmp_path / "dropin.pcd")], capture_output=True, text=True, timeout=100)
    print(p.stdout)
    assert p.returncode == 0, p.stderr + p.stdout[-2000:]
    assert "surface normals as expected" in p.stdout and "normals identical" in p.stdout
    assert "read back" in p.stdout and "refused" in p.stdout
    m = re.search(r"k search 9: (\d+) normals, (\d+) short", p.stdout)
    assert m and int(m.group(1)) == 3200 and int(m.group(2)) == 0


def test_app_estimates_and_saves_the_maps_normals(tmp_path):
    exe = os.path.join(BIN, "KFsphereSLAM")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build()"
    args = ["--synthetic-frames", "0,4,8,12,16", "1"]
    pcd = str(tmp_path / "map.pcd")
    plain = subprocess.run([exe, *args], capture_output=True, text=True, timeout=100)
    run = subprocess.run([exe, *args, "--map-normals", "20,0.25", "--save-map", pcd], capture_output=True, text=True, timeout=100)
    assert plain.returncode == 0 and run.returncode == 0, plain.stderr + run.stderr
    lines = run.stdout.splitlines()
    m = re.fullmatch(r"map normals: (\d+) points, (\d+) short, ([0-9.]+) neighbours on average", lines[-1])
    assert m, lines[-3:]
    print(lines[-1])
    assert "\n".join(lines[:-1]) == plain.stdout.rstrip("\n")        # the flags add one line and change nothing else
    sizes = re.search(r"global map: (\d+) points at the chained poses, (\d+) at the optimised poses", run.stdout)
    n = int(m.group(1))
    assert n == int(sizes.group(2)) and 0 <= int(m.group(2)) < n and 3.0 <= float(m.group(3)) <= 20.0
    xyz, rgba, nrm, curv = R.pcd_read_normals(pcd)
    assert len(xyz) == n and np.isfinite(xyz).all()
    ok = np.isfinite(nrm).all(1)
    assert ok.sum() == n - int(m.group(2)) and np.array_equal(np.isfinite(curv), ok)
    length = np.sqrt((nrm[ok].astype(np.float64) ** 2).sum(1))
    print(f"{int(ok.sum())} normals, |n| - 1 within {np.abs(length - 1).max():.2e}")
    assert np.abs(length - 1).max() <= 2.0 ** -22
    assert (curv[ok] >= 0).all() and (curv[ok] <= 1 / 3 + 1e-6).all()
    # without --map-normals the map is saved as a plain cloud
    pcd2 = str(tmp_path / "plain.pcd")
    run2 = subprocess.run([exe, *args, "--save-map", pcd2], capture_output=True, text=True, timeout=100)
    assert run2.returncode == 0 and run2.stdout == plain.stdout
    px, pc, w, h = R.pcd_read(pcd2)
    assert (w, h) == (n, 1) and px.tobytes() == xyz.tobytes() and pc.tobytes() == rgba.tobytes()
