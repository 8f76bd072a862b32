"""The map step's point-cloud filters, host side (no GPU): a numpy model of their semantics, a hand-computed
known-answer test of the model itself, r360_cloud_filter_euclidean against the model, the new C-ABI symbol, and the
drop-in call sequence of the map step (tests/dropin/global_map_dropin.cpp) compiled with g++ alone.

The model states the three semantics of DESIGN.md §5b in plain numpy (the voxel grid is the statement a device
voxel pass will be checked against; the library does not provide one yet):
  euclid     keep a point iff x, y, z are finite and -2 <= x <= 1, -box <= y, z <= box (float32 compares), in order;
  transform  m(k,0)*x + m(k,1)*y + m(k,2)*z + m(k,3), each product and sum rounded to float32, left to right;
  voxel      key = floor(p * float32(1 / leaf)) in float32; per key the float64 mean rounded to float32 and the
             integer floor of the r / g / b means, alpha 0; output sorted lexicographically on (k, j, i)."""
import os
import subprocess

import numpy as np

import rgbd360_amd as R


# ------------------------------------------------------------------ the model
def euclid_model(xyz, rgba, box=4.0, x_min=-2.0, x_max=1.0):
    p = np.asarray(xyz, np.float32)
    b = np.float32(box)
    with np.errstate(invalid="ignore"):
        keep = (np.isfinite(p).all(1) & (p[:, 0] >= np.float32(x_min)) & (p[:, 0] <= np.float32(x_max))
                & (p[:, 1] >= -b) & (p[:, 1] <= b) & (p[:, 2] >= -b) & (p[:, 2] <= b))
    return p[keep], np.asarray(rgba, np.uint32)[keep]


def transform_model(xyz, pose):
    """pcl::transformPointCloud on finite points; every operation rounds to float32, no fused multiply-add."""
    p = np.asarray(xyz, np.float32)
    m = np.asarray(pose, np.float32)
    out = np.empty_like(p)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(3):
            a = m[k, 0] * x
            a = a + m[k, 1] * y
            a = a + m[k, 2] * z
            out[:, k] = a + m[k, 3]
    return out


def voxel_keys(xyz, leaf=0.05):
    """(i, j, k) per point: floor(p * float32(1 / leaf)), the product in float32."""
    inv = np.float32(1.0) / np.float32(leaf)
    return np.floor(np.asarray(xyz, np.float32) * inv).astype(np.int64)


def voxel_model(xyz, rgba, leaf=0.05):
    """Returns (ijk [m,3] sorted on (k, j, i), mean64 [m,3], xyz32 [m,3], rgba [m], counts [m])."""
    p = np.asarray(xyz, np.float32)
    c = np.asarray(rgba, np.uint32)
    fin = np.isfinite(p).all(1)
    p, c = p[fin], c[fin]
    ijk = voxel_keys(p, leaf)
    order = np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2]))      # primary k, then j, then i
    ijk, p, c = ijk[order], p[order], c[order]
    new = np.ones(len(p), bool)
    new[1:] = (ijk[1:] != ijk[:-1]).any(1)
    start = np.flatnonzero(new)
    counts = np.diff(np.append(start, len(p)))
    if len(p) == 0:
        z = np.zeros((0, 3))
        return ijk, z, z.astype(np.float32), c, counts
    mean64 = np.add.reduceat(p.astype(np.float64), start, axis=0) / counts[:, None]
    ch = [np.add.reduceat(((c >> s) & 255).astype(np.int64), start) // counts for s in (16, 8, 0)]
    out_c = (ch[0] << 16 | ch[1] << 8 | ch[2]).astype(np.uint32)
    return ijk[start], mean64, mean64.astype(np.float32), out_c, counts


# ------------------------------------------------------------------ tests
def test_filter_symbol_is_bound():
    assert "r360_cloud_filter_euclidean" in R.ABI_SYMBOLS
    assert hasattr(R.lib(), "r360_cloud_filter_euclidean")
    ex, ec = R.FilterPointCloud().filterEuclidean(np.array([[0, 0, 0], [0, 5, 0], [1.5, 0, 0]], np.float32),
                                                  np.array([1, 2, 3], np.uint32))
    assert ex.tolist() == [[0, 0, 0]] and ec.tolist() == [1]
    ex, _ = R.FilterPointCloud(0.05, 6.0).filterEuclidean(np.array([[0, 0, 0], [0, 5, 0], [1.5, 0, 0]], np.float32))
    assert ex.tolist() == [[0, 0, 0], [0, 5, 0]]


def test_model_known_answer():
    """6 points, 3 voxels, worked by hand at leaf 0.05 (float32(1 / 0.05f) = 20):
      A (0.01, 0.01, 0.01), (0.03, 0.02, 0.04)        -> voxel ( 0,  0, 0), mean ( 0.02,  0.015, 0.025)
      B (-0.01, 0.01, 0.01), (-0.03, 0.03, 0.02)      -> voxel (-1,  0, 0): floor(-0.2) = -1, truncation would give 0
      C (0.12, -0.07, 0.26), (0.14, -0.06, 0.27)      -> voxel ( 2, -2, 5): floor(2.4), floor(-1.4), floor(5.2)
    ascending (k, j, i): B, A, C.  Colours: A (10,20,30)+(11,21,33) -> (10,20,31); B (255,0,1)+(0,255,2) ->
    (127,127,1); C (100,100,100)+(101,103,100) -> (100,101,100); the inputs' alpha 255 is dropped."""
    assert np.float32(1.0) / np.float32(0.05) == np.float32(20.0)
    pack = lambda r, g, b: 255 << 24 | r << 16 | g << 8 | b
    xyz = np.array([[0.12, -0.07, 0.26], [0.01, 0.01, 0.01], [-0.01, 0.01, 0.01], [0.03, 0.02, 0.04],
                    [0.14, -0.06, 0.27], [-0.03, 0.03, 0.02]], np.float32)
    rgba = np.array([pack(100, 100, 100), pack(10, 20, 30), pack(255, 0, 1), pack(11, 21, 33), pack(101, 103, 100),
                     pack(0, 255, 2)], np.uint32)
    ijk, mean64, xyz32, c, counts = voxel_model(xyz, rgba)
    assert ijk.tolist() == [[-1, 0, 0], [0, 0, 0], [2, -2, 5]]
    assert counts.tolist() == [2, 2, 2]
    want = np.array([[-0.02, 0.02, 0.015], [0.02, 0.015, 0.025], [0.13, -0.065, 0.265]])
    assert np.abs(mean64 - want).max() < 1e-8            # the inputs are float32 roundings of the decimals
    assert np.abs(xyz32 - want).max() < 2e-8
    assert c.tolist() == [127 << 16 | 127 << 8 | 1, 10 << 16 | 20 << 8 | 31, 100 << 16 | 101 << 8 | 100]
    # a non-finite point is dropped, nothing else changes
    ijk2, _, xyz2, c2, _ = voxel_model(np.vstack([xyz, [[np.nan, 0, 0]], [[0, np.inf, 0]]]).astype(np.float32),
                                       np.append(rgba, [1, 2]).astype(np.uint32))
    assert np.array_equal(ijk2, ijk) and np.array_equal(xyz2, xyz32) and np.array_equal(c2, c)


def test_filter_euclidean_matches_model():
    rng = np.random.default_rng(5)
    n = 10000
    xyz = rng.uniform(-6, 6, (n, 3)).astype(np.float32)
    xyz[::7, 0] = rng.uniform(-2.5, 1.5, len(xyz[::7])).astype(np.float32)
    special = [np.nan, np.inf, -np.inf, -2.0, 1.0, 4.0, -4.0, np.nextafter(np.float32(-2), np.float32(-3)),
               np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(4), np.float32(5)),
               np.nextafter(np.float32(-4), np.float32(-5)), 0.0, -0.0]
    k = 0
    for axis in range(3):
        for v in special:
            for rep in range(4):                       # each special value with in-box and random other coordinates
                row = 100 + k
                if rep < 2:
                    xyz[row] = rng.uniform(-0.9, 0.9, 3).astype(np.float32)
                xyz[row, axis] = v
                k += 1
    rgba = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    want_xyz, want_rgba = euclid_model(xyz, rgba)
    assert 0 < len(want_xyz) < n
    # the closed ends are kept, the next floats beyond them are not
    edge = np.array([[-2, 4, -4], [1, -4, 4], [np.nextafter(np.float32(1), np.float32(2)), 0, 0]], np.float32)
    assert len(euclid_model(edge, np.zeros(3, np.uint32))[0]) == 2
    got_xyz, got_rgba = R.filter_euclidean(xyz, rgba)
    assert got_xyz.shape == want_xyz.shape
    assert np.array_equal(got_xyz.view(np.uint32), want_xyz.view(np.uint32))      # order and bits
    assert np.array_equal(got_rgba, want_rgba)
    got_e, _ = R.filter_euclidean(edge, np.zeros(3, np.uint32))
    assert np.array_equal(got_e, edge[:2])
    # another box, and no colours
    w2, _ = euclid_model(xyz, rgba, box=1.5)
    g2, none = R.filter_euclidean(xyz, None, box=1.5)
    assert none is None and np.array_equal(g2.view(np.uint32), w2.view(np.uint32))


def _transform_program(root, tmp_path, flags):
    """Builds a small program that runs r360::transformPointCloud on points from stdin (header-only: no library)."""
    src = tmp_path / "xform.cpp"
    src.write_text("""#include <rgbd360/rgbd360.h>
#include <cstdio>
int main() {
    r360::Matrix4f T;
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) if (std::scanf("%f", &T(r, c)) != 1) return 1;
    r360::PointCloud in, out;
    float x, y, z;
    while (std::scanf("%f %f %f", &x, &y, &z) == 3) { in.xyz.push_back(x); in.xyz.push_back(y); in.xyz.push_back(z); in.rgba.push_back(0); }
    in.width = int(in.size()); in.height = 1;
    r360::transformPointCloud(in, out, T);
    for (size_t i = 0; i < out.size(); ++i) std::printf("%a %a %a\\n", out.xyz[3 * i], out.xyz[3 * i + 1], out.xyz[3 * i + 2]);
    return 0;
}
""")
    exe = tmp_path / "xform"
    p = subprocess.run(["g++", "-std=c++17", *flags, "-Wall", "-Wextra", "-Werror", f"-I{root}/include", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(exe)


def test_transform_point_cloud_matches_model(root, tmp_path):
    """r360::transformPointCloud == the model bit for bit, also when the compiler may fuse multiply-adds
    (-O2 -mfma -ffp-contract=fast): the function opts out of contraction."""
    rng = np.random.default_rng(2)
    pts = rng.uniform(-5, 5, (2000, 3)).astype(np.float32)
    a = 0.37
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32) @ np.array(
        [[1, 0, 0], [0, np.cos(0.2), -np.sin(0.2)], [0, np.sin(0.2), np.cos(0.2)]], np.float32)
    T[:3, 3] = (0.013, 0.2, -0.1)
    want = transform_model(pts, T)
    text = "\n".join(" ".join(float(v).hex() for v in row) for row in T) + "\n" + "\n".join(
        " ".join(float(v).hex() for v in row) for row in pts) + "\n"
    flagsets = [["-O0"], ["-O2", "-mfma", "-ffp-contract=fast"]]
    if "fma" not in open("/proc/cpuinfo").read():
        flagsets = flagsets[:1]
    for flags in flagsets:
        exe = _transform_program(root, tmp_path, flags)
        p = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert p.returncode == 0
        got = np.array([[float.fromhex(v) for v in line.split()] for line in p.stdout.splitlines()], np.float32)
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), flags


def test_global_map_call_sequence_compiles(root):
    """tests/dropin/global_map_dropin.cpp — a FilterPointCloud with the reference's defaults, filterEuclidean on a
    frame's cloud, transformPointCloud and += — compiles with g++ alone, warning-free."""
    for opt in ("-O0", "-O2"):
        p = subprocess.run(["g++", "-std=c++17", opt, "-fsyntax-only", "-Wall", "-Wextra", "-Werror", f"-I{root}/include",
                            f"{root}/tests/dropin/global_map_dropin.cpp"], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
    src = open(os.path.join(root, "tests", "dropin", "global_map_dropin.cpp")).read()
    for call in ("FilterPointCloud filter", "filterEuclidean(", "transformPointCloud(", "+="):
        assert call in src, call
