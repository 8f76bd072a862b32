"""The RANSAC plane segmentation through the C++ façade: the PCL-shaped call sequence and the planes-off-then-clusters
recipe (tests/dropin/sac_dropin.cpp) and KFsphereSLAM --map-planes / --save-planes / --remove-planes."""
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
    exe = os.path.join(BIN, "sac_dropin")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build()"
    p = subprocess.run([exe, str(tmp_path / "dropin.pcd")], capture_output=True, text=True, timeout=100)
    print(p.stdout)
    assert p.returncode == 0, p.stderr + p.stdout[-2000:]
    assert "plane: 1200 inliers after 128 hypotheses" in p.stdout and "coefficients as expected" in p.stdout
    assert "perpendicular to x: 900 inliers" in p.stdout and "parallel to x: 1200 inliers" in p.stdout
    assert "other models refused" in p.stdout and "device map: 2249 points, 2 planes 1200 900" in p.stdout
    assert "read back" in p.stdout and "planes removed: 149 points left, plane labels refused" in p.stdout
    assert "clusters on the rest: 1 of 144 points" in p.stdout


def test_app_peels_planes_saves_them_and_clusters_the_rest(tmp_path):
    exe = os.path.join(BIN, "KFsphereSLAM")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build()"
    args = ["--synthetic-frames", "0,4,8,12,16", "1"]
    pcd = str(tmp_path / "planes.pcd")
    run = subprocess.run([exe, *args, "--map-planes", "0.05,100", "--save-planes", pcd, "--remove-planes", "--map-clusters",
                          "0.1,50"], capture_output=True, text=True, timeout=100)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    print("\n".join(lines[-3:]))
    sizes = re.search(r"global map: (\d+) points at the chained poses, (\d+) at the optimised poses", run.stdout)
    m = re.fullmatch(r"map planes: (\d+) points, (\d+) planes, (\d+) points in planes, largest (\d+)", lines[-2])
    c = re.fullmatch(r"map clusters: (\d+) points, (\d+) components, (\d+) kept, largest (\d+)", lines[-1])
    assert sizes and m and c, lines[-3:]
    n, planes, in_planes, largest = (int(v) for v in m.groups())
    assert n == int(sizes.group(2)) and 1 <= planes <= 8 and largest <= in_planes <= n
    xyz, rgba, labels = R.read_pcd_labels(pcd)
    assert len(xyz) == n and np.isfinite(xyz).all()
    assert labels.min() >= -1 and labels.max() == planes - 1
    counts = np.bincount(labels[labels >= 0], minlength=planes)
    assert counts.min() >= 100 and counts.max() == largest and counts.sum() == in_planes
    assert int(c.group(1)) == n - in_planes                       # the clusters are those of what the planes left
    # the refused combinations exit 1 with the usage text
    for extra in (["--remove-planes"], ["--save-planes", pcd],
                  ["--map-normals", "20,0.25", "--map-planes", "0.05,100", "--remove-planes", "--map-clusters", "0.1,50,15"],
                  ["--map-planes", "0.05"]):
        bad = subprocess.run([exe, *args, *extra], capture_output=True, text=True, timeout=100)
        assert bad.returncode == 1 and "usage:" in bad.stderr, extra
