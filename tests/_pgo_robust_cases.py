"""Pose graphs with one wrong loop edge, for the robust-kernel tests (CPU and GPU): the 9-, 33- and 65-vertex graphs
of _pgo_cases' recipe on the figure-eight path, each with one last edge (i, j) whose measurement is the true
relative pose composed with a fixed wrong transform (0.4 rad about y, then (1.0, -0.7, 0.5) m) at an ordinary
information matrix: what PbMap matching between two alike rooms would hand the back end.

At import the model runs once per case without a kernel, with Huber delta = 1 and with Cauchy delta = 3 on every
edge; the results are kept (get(name)) and these are asserted, on the CPU:
  * no decision of any of the three runs is undecided (pgo_model.undecided);
  * without a kernel the worst translation error is more than twice that of the chained start;
  * with either kernel it is below that of the chained start;
  * at either robust optimum the wrong edge's chi2 is more than 100 times every other edge's.
"""
import numpy as np

import _pgo_cases as Cs
import pgo_model as M
import pgo_robust_model as RM

WRONG = {"n9": (2, 7), "n33": (5, 27), "n65": (10, 50)}
ALL = list(WRONG)
KERNELS = {"huber": (RM.HUBER, 1.0), "cauchy": (RM.CAUCHY, 3.0)}


def wrong_transform():
    T = np.eye(4)
    T[:3, :3] = M.exp_so3([0.0, 0.4, 0.0])
    T[:3, 3] = [1.0, -0.7, 0.5]
    return T


def _base(name):
    if name == "n33":
        truth = [Cs.path_pose(8 * k) for k in range(33)]
        return Cs._chain(np.random.default_rng(1033), truth, [(0, 16), (0, 32), (8, 24)]), truth
    n = int(name[1:])
    return Cs.build_sized(n, *Cs.SIZED[n])


def worst_error(poses, truth):
    return max(float(np.linalg.norm(a[:3, 3] - b[:3, 3])) for a, b in zip(poses, truth))


class Case:
    def __init__(self, name):
        g, truth = _base(name)
        self.name, self.truth = name, truth
        self.clean = g.copy()                     # the graph without the wrong edge
        i, j = WRONG[name]
        g.add_edge(i, j, Cs.mul4(M.rel4(truth[i], truth[j]), wrong_transform()), Cs.info(np.random.default_rng(5)))
        self.graph = g
        self.wrong = len(g.edges) - 1             # the wrong edge's index
        m = len(g.edges)
        self.err_start = worst_error(g.poses, truth)
        self.runs = {"none": RM.optimize(g)}
        for key, kd in KERNELS.items():
            self.runs[key] = RM.optimize(g, [kd] * m)
        for key, (poses, st) in self.runs.items():
            bad = M.undecided(st)
            assert not bad, (name, key, bad)
        self.err = {key: worst_error(poses, truth) for key, (poses, _) in self.runs.items()}
        assert self.err["none"] > 2.0 * self.err_start, (name, self.err, self.err_start)
        self.chi2 = {}
        for key, kd in KERNELS.items():
            assert self.err[key] < self.err_start, (name, key, self.err, self.err_start)
            c, _ = RM.edge_stats(g, [kd] * m, poses=self.runs[key][0])
            self.chi2[key] = c
            others = np.delete(c, self.wrong)
            assert c[self.wrong] > 100.0 * float(np.max(others)), (name, key, c[self.wrong], float(np.max(others)))


CASES = {name: Case(name) for name in ALL}   # at import: nine model runs, well under a second in all


def get(name):
    return CASES[name]
