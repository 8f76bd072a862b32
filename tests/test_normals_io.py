"""PCD files of clouds with normals (r360_pcd_write_normals / r360_pcd_read_normals, host only): the header, and a round
trip in every mode that returns the normals and the curvature byte for byte."""
import ctypes as C

import numpy as np
import pytest

import rgbd360_amd as R

EINVAL = -2
MODES = [R.PCD_ASCII, R.PCD_BINARY, R.PCD_BINARY_COMPRESSED]


def _cloud(n=301, seed=4):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
    rgba = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    curv = rng.uniform(0, 1 / 3, n).astype(np.float32)
    # what an estimation leaves: dropped and short rows are NaN; exact values, a zero of either sign, tiny and
    # denormal ones, and floats that eight printed digits would not return
    nrm[5] = np.nan
    curv[5] = np.nan
    nrm[6] = [0.0, -0.0, 1.0]
    nrm[7] = [np.float32(1e-30), np.float32(-1e-42), -1.0]
    nrm[8] = np.float32([0.1, 0.2, 0.3]) + np.float32(2.0 ** -26)
    curv[6:9] = [0.0, np.float32(1e-39), np.nextafter(np.float32(1 / 3), np.float32(1))]
    xyz[5] = np.nan
    return xyz, rgba, nrm, curv


def _header(path):
    lines = []
    with open(path, "rb") as f:
        for raw in f:
            line = raw.decode("ascii", "replace").rstrip("\n")
            lines.append(line)
            if line.startswith("DATA"):
                break
    return lines


@pytest.mark.parametrize("mode", MODES)
def test_round_trip_returns_the_bytes(tmp_path, mode):
    xyz, rgba, nrm, curv = _cloud()
    path = str(tmp_path / "cloud.pcd")
    R.pcd_write_normals(path, xyz, rgba, nrm, curv, mode)
    h = _header(path)
    n = len(xyz)
    assert h[1:] == ["VERSION 0.7", "FIELDS x y z rgba normal_x normal_y normal_z curvature", "SIZE 4 4 4 4 4 4 4 4",
                     "TYPE F F F U F F F F", "COUNT 1 1 1 1 1 1 1 1", f"WIDTH {n}", "HEIGHT 1", "VIEWPOINT 0 0 0 1 0 0 0",
                     f"POINTS {n}", "DATA " + ["ascii", "binary", "binary_compressed"][mode]]
    gx, gc, gn, gv = R.pcd_read_normals(path)
    assert gn.tobytes() == nrm.tobytes() and gv.tobytes() == curv.tobytes()
    assert gc.tobytes() == rgba.tobytes()
    if mode == R.PCD_ASCII:                                  # eight digits, as the plain writer prints coordinates
        assert np.allclose(gx, xyz, rtol=1e-7, atol=0, equal_nan=True)
    else:
        assert gx.tobytes() == xyz.tobytes()
    # the plain reader takes the same file as a PointXYZRGBA cloud
    px, pc, w, hgt = R.pcd_read(path)
    assert (w, hgt) == (n, 1) and pc.tobytes() == rgba.tobytes() and px.tobytes() == gx.tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_empty_partial_and_missing_arrays(tmp_path, mode):
    L = R.lib()
    path = str(tmp_path / "c.pcd")
    z3, z1 = np.zeros((0, 3), np.float32), np.zeros(0, np.float32)
    R.pcd_write_normals(path, z3, None, z3, z1, mode)
    gx, gc, gn, gv = R.pcd_read_normals(path)
    assert len(gx) == len(gc) == len(gn) == len(gv) == 0
    xyz, rgba, nrm, curv = _cloud(40)
    # no colours, no curvature: written as 0
    assert L.r360_pcd_write_normals(path.encode(), R._fptr(xyz), None, R._fptr(nrm), None, 40, mode) == 0
    gx, gc, gn, gv = R.pcd_read_normals(path)
    assert not gc.any() and not gv.view(np.uint32).any() and gn.tobytes() == nrm.tobytes()
    # a short capacity reads the first points and still reports the file's size
    R.pcd_write_normals(path, xyz, rgba, nrm, curv, mode)
    n = C.c_size_t()
    pn, pv = np.zeros((10, 3), np.float32), np.zeros(10, np.float32)
    assert L.r360_pcd_read_normals(path.encode(), None, None, R._fptr(pn), R._fptr(pv), 10, C.byref(n)) == 0
    assert n.value == 40 and pn.tobytes() == nrm[:10].tobytes() and pv.tobytes() == curv[:10].tobytes()


def test_errors(tmp_path):
    L = R.lib()
    xyz, rgba, nrm, curv = _cloud(12)
    path = str(tmp_path / "c.pcd").encode()
    fx, fn, fv = R._fptr(xyz), R._fptr(nrm), R._fptr(curv)
    assert L.r360_pcd_write_normals(None, fx, None, fn, fv, 12, 0) == EINVAL
    assert L.r360_pcd_write_normals(path, None, None, fn, fv, 12, 0) == EINVAL
    assert L.r360_pcd_write_normals(path, fx, None, fn, fv, 12, 3) == EINVAL
    assert L.r360_pcd_write_normals(path, fx, None, fn, fv, 12, -1) == EINVAL
    n = C.c_size_t()
    assert L.r360_pcd_read_normals(None, None, None, None, None, 0, C.byref(n)) == EINVAL
    assert L.r360_pcd_read_normals(str(tmp_path / "missing.pcd").encode(), None, None, None, None, 0, C.byref(n)) < 0
    # a plain PointXYZRGBA file has no normals to read
    plain = str(tmp_path / "plain.pcd")
    R.pcd_write(plain, xyz, rgba, 12, 1, R.PCD_BINARY)
    assert L.r360_pcd_read_normals(plain.encode(), None, None, None, None, 0, C.byref(n)) < 0
    assert b"normal_x" in L.r360_last_error()
    with pytest.raises(RuntimeError):
        R.pcd_read_normals(plain)
