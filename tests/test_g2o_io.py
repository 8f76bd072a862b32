"""g2o text files (r360_g2o_write / r360_g2o_read): host-only, no GPU."""
import numpy as np
import pytest

import rgbd360_amd as R

import _pgo_cases as Cs
import pgo_model as M


def _write_case(path, name):
    c = Cs.get(name)
    g = c.graph
    R.g2o_write(str(path), g.poses, [int(f) for f in g.fixed], g.edges)
    return g


@pytest.mark.parametrize("name", ["n9", "n65", "big_rotations", "fixed8", "reversed"])
def test_round_trip(tmp_path, name):
    """Write, read, write again: the same bytes.  Information matrices, indices and FIX lines come back exactly,
    poses within 1e-14 per entry (the quaternion round trip and its 2^-48 lattice)."""
    a, b = tmp_path / "a.g2o", tmp_path / "b.g2o"
    g = _write_case(a, name)
    poses, fixed, edges = R.g2o_read(str(a))
    R.g2o_write(str(b), poses, fixed, edges)
    assert a.read_bytes() == b.read_bytes()
    assert [bool(f) for f in fixed] == g.fixed
    assert len(edges) == len(g.edges)
    worst = max(float(np.max(np.abs(p - q))) for p, q in zip(poses, g.poses))
    for (i, j, Z, Om), (gi, gj, gZ, gOm) in zip(edges, g.edges):
        assert (i, j) == (gi, gj)
        assert np.array_equal(Om, gOm)
        worst = max(worst, float(np.max(np.abs(Z - gZ))))
        assert np.array_equal(Z[:3, 3], gZ[:3, 3])
    print(f"{name}: max pose entry error after the round trip {worst:.2e}")
    assert worst <= 1e-14
    for p, q in zip(poses, g.poses):
        assert np.array_equal(p[:3, 3], q[:3, 3])


def test_format(tmp_path):
    """The lines g2o's saveGraph writes: tags, field counts, %.17g, Shepperd's quaternion with qw >= 0."""
    p = tmp_path / "a.g2o"
    g = _write_case(p, "n3")
    lines = p.read_text().splitlines()
    v = [l.split() for l in lines if l.startswith("VERTEX_SE3:QUAT")]
    e = [l.split() for l in lines if l.startswith("EDGE_SE3:QUAT")]
    assert len(v) == 3 and all(len(x) == 9 for x in v)
    assert len(e) == len(g.edges) and all(len(x) == 3 + 7 + 21 for x in e)
    assert [l for l in lines if l.startswith("FIX")] == ["FIX 0"]
    for x, T in zip(v, g.poses):
        assert [float(s) for s in x[2:5]] == list(T[:3, 3])
        q = np.array([float(s) for s in x[5:9]])
        assert q[3] >= 0 and abs(np.linalg.norm(q) - 1) < 1e-15
        assert np.max(np.abs(q - M.quat_of(T[:3, :3]))) < 1e-14
    up = [float(s) for s in e[0][10:]]
    assert up == [g.edges[0][3][r, c] for r in range(6) for c in range(r, 6)]


def test_half_turn_and_negative_trace(tmp_path):
    """Every branch of Shepperd's method, and qw = 0."""
    poses = []
    for ax in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 2, 3]):
        a = np.array(ax, float) / np.linalg.norm(ax)
        for th in (np.pi, 3.0, 2.0, 1e-9):
            T = np.eye(4)
            T[:3, :3] = M.exp_so3(a * th) if th != np.pi else 2 * np.outer(a, a) - np.eye(3)
            poses.append(T)
    a, b = tmp_path / "a.g2o", tmp_path / "b.g2o"
    R.g2o_write(str(a), poses, None, [])
    back, fixed, edges = R.g2o_read(str(a))
    R.g2o_write(str(b), back, fixed, edges)
    assert a.read_bytes() == b.read_bytes()
    assert max(float(np.max(np.abs(p - q))) for p, q in zip(back, poses)) <= 1e-14


@pytest.mark.parametrize("text", [
    "VERTEX_SE3:QUAT 0 0 0 0 0 0 0\n",                                  # a short vertex line
    "PARAMS_SE3OFFSET 0 0 0 0 0 0 0 1\nVERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\n",   # an unknown tag before the first vertex
    "VERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\nEDGE_SE3:QUAT 0 1 0 0 0 0 0 0 1 1 0 0\n",   # a short edge line
    "VERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\nVERTEX_SE3:QUAT 2 0 0 0 0 0 0 1\n",   # ids not 0 .. n-1
    "VERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\nFIX 3\n",                         # FIX of a missing vertex
    "VERTEX_SE3:QUAT 0 0 0 0 x 0 0 1\n",                                # not a number
    "VERTEX_SE3:QUAT 0 0 0 0 0 0 0 0\n",                                # a zero quaternion
])
def test_malformed_files_are_errors(tmp_path, text):
    p = tmp_path / "bad.g2o"
    p.write_text(text)
    with pytest.raises(RuntimeError, match="g2o"):
        R.g2o_read(str(p))


def test_comments_blank_lines_and_later_unknown_tags_are_skipped(tmp_path):
    p = tmp_path / "ok.g2o"
    p.write_text("# a comment\n\nVERTEX_SE3:QUAT 0 1 2 3 0 0 0 1\nSOMETHING_ELSE 1 2 3\nFIX 0")
    poses, fixed, edges = R.g2o_read(str(p))
    assert len(poses) == 1 and list(fixed) == [1] and edges == []
    assert np.array_equal(poses[0][:3, 3], [1, 2, 3]) and np.array_equal(poses[0][:3, :3], np.eye(3))


def test_missing_file_is_an_error(tmp_path):
    with pytest.raises(RuntimeError):
        R.g2o_read(str(tmp_path / "none.g2o"))
