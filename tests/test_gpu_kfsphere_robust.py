"""apps/KFsphereSLAM with --robust, --reject-chi2 and --false-loop, on the out-and-back list of
tests/test_gpu_kfsphere_slam.py (5 keyframes, 3 loop edges):

  (a) a Huber kernel that never bites (--robust huber:1e9) leaves every keyframe line as it is without the flag;
  (b) a wrong loop edge 0 -> 2 at full quadratic weight (--false-loop 0,2) bends the trajectory: the worst optimised
      distance from the path exceeds that of the same run without it.

A third case, rejecting the false edge with --robust cauchy:D --reject-chi2 T, needs a T at least a factor 3 from the
false edge's chi2 on one side and from the largest true loop edge's on the other, both read from run (b).  Run (b)
does not offer it: measured on an MI355X, after the second optimisation the false edge 0 2 has chi2 9.50e8 and the
true edge 0 3 has 3.57e8, after the third 9.56e8 against 3.42e8 (the other true edges: 2.2e6 and 0), a ratio of 2.7
where 9 is needed, because the wrong edge at full weight drags the true edge that closes on the same vertex along.
So that case is not tested here (DESIGN.md §5d has the figures)."""
import functools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "bin", "KFsphereSLAM")
FRAMES = "0,4,8,12,16,12,8,4,0"


@functools.lru_cache(maxsize=None)
def _run(*flags):
    assert os.path.exists(EXE), f"{EXE} missing: run __graft_entry__.build()"
    p = subprocess.run([EXE, "--synthetic-frames", FRAMES, "1", *flags], capture_output=True, text=True, timeout=100)
    assert p.returncode == 0, p.stderr + p.stdout[-2000:]
    return p.stdout


def _lines(out, start):
    rows = [l for l in out.splitlines() if l.startswith(start)]
    return rows


def _worst(out):
    m = re.search(r"worst distance from the path: chain (\S+) m, optimised (\S+) m", out)
    assert m, out[-2000:]
    return float(m.group(1)), float(m.group(2))


def test_bad_flags_print_the_usage():
    assert os.path.exists(EXE), f"{EXE} missing: run __graft_entry__.build()"
    for flags in (["--robust", "tukey:1"], ["--robust", "huber"], ["--robust", "cauchy:0"], ["--reject-chi2", "-1"],
                  ["--false-loop", "2,2"], ["--false-loop", "3"]):
        p = subprocess.run([EXE, "--synthetic-frames", FRAMES, "1", *flags], capture_output=True, text=True, timeout=100)
        assert p.returncode == 1 and "--reject-chi2" in p.stderr and "choose D and T" in p.stderr, (flags, p.stderr)


@pytest.mark.gpu
def test_a_kernel_that_never_bites_leaves_the_keyframes_as_they_are():
    plain, robust = _run(), _run("--robust", "huber:1e9")
    assert _lines(plain, "keyframe ") and _lines(plain, "keyframe ") == _lines(robust, "keyframe ")
    assert _lines(plain, "Optimize graph SLAM") == _lines(robust, "Optimize graph SLAM")
    assert _lines(plain, "global map") == _lines(robust, "global map")
    assert not _lines(plain, "loop edge ") and "LC reject" not in plain      # without a flag: the output of before
    rows = _lines(robust, "loop edge ")
    print("\n".join(rows))
    assert len(rows) >= 3 and all(r.endswith(" weight 1") for r in rows)
    assert [l for l in robust.splitlines() if not l.startswith("loop edge ")] == plain.splitlines()


@pytest.mark.gpu
def test_rejection_deactivates_and_optimises_again():
    """The mechanism alone, with thresholds that need no choosing: T = inf rejects nothing and changes nothing, T = 0
    rejects every loop edge whose chi2 is above 0 right after the optimisation that reported it, and each
    optimisation that rejected something is followed by another."""
    plain, none = _run(), _run("--reject-chi2", "inf")
    assert [l for l in none.splitlines() if not l.startswith("loop edge ")] == plain.splitlines()
    out = _run("--reject-chi2", "0").splitlines()
    rejects = [k for k, l in enumerate(out) if l.startswith("LC reject edge between ")]
    assert rejects
    seen = set()
    for k in rejects:
        m = re.fullmatch(r"LC reject edge between (\d+) and (\d+) chi2 (\S+)", out[k])
        assert m and float(m.group(3)) > 0.0
        assert f"loop edge {m.group(1)} {m.group(2)} chi2 {m.group(3)} weight 1" in out[:k]
        assert (m.group(1), m.group(2)) not in seen                      # an edge is rejected once
        seen.add((m.group(1), m.group(2)))
        nxt = next(l for l in out[k + 1:] if not l.startswith("LC reject"))
        assert nxt.startswith("Optimize graph SLAM")
    n_opt = int(re.search(r"(\d+) optimisations", "\n".join(out)).group(1))
    assert n_opt == sum(l.startswith("Optimize graph SLAM") for l in out) > sum(l.startswith("Optimize") for l in plain.splitlines())
    last = [l for l in out if l.startswith("loop edge ")]
    rejected_rows = [l for l in last[-3:] if tuple(l.split()[2:4]) in seen]
    assert rejected_rows and all(l.endswith(" weight 0") for l in rejected_rows)   # an inactive edge: its chi2, weight 0


@pytest.mark.gpu
def test_a_false_loop_at_full_weight_bends_the_trajectory():
    plain, bent = _run(), _run("--false-loop", "0,2")
    assert "LC Add false edge between 0 and 2" in bent
    loops = lambda out: int(re.search(r"(\d+) keyframes, (\d+) loop edges", out).group(2))
    assert loops(bent) == loops(plain) + 1
    print("\n".join(l for l in bent.splitlines() if l.startswith(("Optimize graph SLAM", "loop edge "))))
    (c0, w0), (c1, w1) = _worst(plain), _worst(bent)
    print(f"worst optimised distance from the path: {w0:.4f} m without the false loop, {w1:.4f} m with it (chain {c0:.4f} m)")
    assert c0 == c1 and w1 > w0
    assert _lines(bent, "loop edge 0 2 chi2 ") and "LC reject" not in bent
