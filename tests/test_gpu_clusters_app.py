"""The cluster extraction through the C++ façade: the PCL-shaped call sequence (tests/dropin/clusters_dropin.cpp) and
KFsphereSLAM --clean-map cluster:... / --map-clusters / --save-clusters."""
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
    exe = os.path.join(BIN, "clusters_dropin")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build()"
    p = subprocess.run([exe, str(tmp_path / "dropin.pcd")], capture_output=True, text=True, timeout=100)
    print(p.stdout)
    assert p.returncode == 0, p.stderr + p.stdout[-2000:]
    assert "plain: 2 clusters of 7 components 1800 144" in p.stdout and "records as expected" in p.stdout
    assert "with normals: 3 clusters 900 900 144" in p.stdout and "labels and records identical" in p.stdout
    assert "read back" in p.stdout and "1944 points left, labels refused" in p.stdout


def test_app_cleans_clusters_and_saves_the_maps_clusters(tmp_path):
    exe = os.path.join(BIN, "KFsphereSLAM")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build()"
    args = ["--synthetic-frames", "0,4,8,12,16", "1"]
    pcd = str(tmp_path / "clusters.pcd")
    run = subprocess.run([exe, *args, "--clean-map", "cluster:0.1,50", "--map-normals", "20,0.25", "--map-clusters", "0.1,50,15",
                          "--save-clusters", pcd], capture_output=True, text=True, timeout=100)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    print("\n".join(lines[-3:]))
    sizes = re.search(r"global map: (\d+) points at the chained poses, (\d+) at the optimised poses", run.stdout)
    c = re.fullmatch(r"map cleaned: (\d+) -> (\d+) points \((\d+) components, (\d+) kept\)", lines[-3])
    assert c and re.match(r"map normals: ", lines[-2]), lines[-3:]
    m = re.fullmatch(r"map clusters: (\d+) points, (\d+) components, (\d+) kept, largest (\d+)", lines[-1])
    assert m, lines[-3:]
    before, after, comps, kept = (int(v) for v in c.groups())
    assert before == int(sizes.group(2)) and 0 < after <= before and 1 <= kept <= comps
    n, comps2, kept2, largest = (int(v) for v in m.groups())
    assert n == after and 1 <= kept2 <= comps2 and 50 <= largest <= n
    assert comps2 >= kept                                          # the normals only cut edges of the cleaned map's pieces
    xyz, rgba, labels = R.read_pcd_labels(pcd)
    assert len(xyz) == n and np.isfinite(xyz).all()
    assert labels.min() >= -1 and labels.max() == kept2 - 1
    counts = np.bincount(labels[labels >= 0], minlength=kept2)
    assert counts[0] == largest and (np.diff(counts) <= 0).all() and counts.min() >= 50
    # an angle without --map-normals is refused with the usage text
    bad = subprocess.run([exe, *args, "--map-clusters", "0.1,50,15"], capture_output=True, text=True, timeout=100)
    assert bad.returncode == 1 and "usage:" in bad.stderr
