"""Shared pose graphs of the pose-graph tests (CPU and GPU), all deterministic, on the benchmark's figure-eight
path (r360_synth_path_pose restated in float64: closed over 256 frames, crossing itself at frame 128).

A sized case has chain edges with 1 cm / 3 mrad noise, loop edges with a fifth of it and random SPD information
matrices (about 1e4 on translation, 1e5 on rotation); its initial poses are the chain's product.  get(name) runs
the model once per case, keeps the result and asserts that every accept / reject and stop decision of the model
is decided: at least 1e-9 of F away from its threshold (pgo_model.undecided).
"""
import functools

import numpy as np

import pgo_model as M

SIZED = {   # n: (stride, loop edges)
    2: (8, []),
    3: (8, [(0, 2)]),
    9: (32, [(0, 4), (0, 8)]),
    65: (4, [(0, 32), (0, 64), (16, 48)]),
    257: (1, [(0, 128), (0, 256), (64, 192), (1, 255)]),
    513: (1, [(0, 128), (0, 256), (64, 192), (1, 255), (128, 384), (0, 512), (256, 512)]),
}
CRAFTED = ["hub", "duplicates", "reversed", "fixed8", "exact_chain", "big_rotations", "small_angles"]
SALT = {"big_rotations": 1}   # the unsalted draw leaves the model's last accept within 1e-12 of F: not usable
ALL = [f"n{n}" for n in SIZED] + CRAFTED


def path_pose(frame):
    w = 2 * np.pi * frame / 256.0
    yaw = 0.35 * np.sin(w + 0.7)
    c, s = np.cos(yaw), np.sin(yaw)
    T = np.eye(4)
    T[:3, :3] = [[1, 0, 0], [0, c, -s], [0, s, c]]
    T[:3, 3] = [0.0, 2.4 * np.sin(w), 1.6 * np.sin(2 * w)]
    return T


def mul4(A, B):
    T = np.eye(4)
    T[:3, :3] = M.mul3(A[:3, :3], B[:3, :3])
    T[:3, 3] = M.mul3(A[:3, :3], B[:3, 3]) + A[:3, 3]
    return T


def noise4(rng, st, sr):
    T = np.eye(4)
    T[:3, :3] = M.exp_so3(rng.normal(0, sr, 3))
    T[:3, 3] = rng.normal(0, st, 3)
    return T


def info(rng):
    A = rng.normal(0, 1, (6, 6))
    W = A @ A.T / 6.0 + np.eye(6)
    s = np.array([100.0] * 3 + [316.0] * 3)
    Om = W * s[:, None] * s[None, :]
    return 0.5 * (Om + Om.T)


def measure(rng, Ti, Tj, st, sr):
    return mul4(M.rel4(Ti, Tj), noise4(rng, st, sr))


class Case:
    def __init__(self, name, graph, truth):
        self.name, self.graph, self.truth = name, graph, truth
        self.poses, self.stats = M.optimize(graph)
        bad = M.undecided(self.stats)
        assert not bad, (name, bad)


def _chain(rng, truth, loops, st=0.01, sr=0.003, fixed=()):
    g = M.Graph()
    Z = [measure(rng, truth[k], truth[k + 1], st, sr) for k in range(len(truth) - 1)]
    T = truth[0].copy()
    g.add_vertex(T)
    for k, z in enumerate(Z):
        T = mul4(T, z)
        g.add_vertex(T, (k + 1) in fixed)
    for k, z in enumerate(Z):
        g.add_edge(k, k + 1, z, info(rng))
    for (i, j) in loops:
        g.add_edge(i, j, measure(rng, truth[i], truth[j], st / 5, sr / 5), info(rng))
    return g


def build_sized(n, stride, loops):
    """The sized recipe without the model run (tools/pgo_bench.py builds its 2049-vertex graph with it)."""
    rng = np.random.default_rng(1000 + n)
    truth = [path_pose(k * stride) for k in range(n)]
    g = _chain(rng, truth, loops)
    if not loops:   # a chain alone: its edges are the relative poses of the chained vertices, so F == 0 exactly
        g.edges = [(i, j, M.rel4(g.poses[i], g.poses[j]), Om) for (i, j, Z, Om) in g.edges]
    return g, truth


def _sized(n):
    return build_sized(n, *SIZED[n])


def _scattered(rng, truth, st=0.03, sr=0.01):
    g = M.Graph()
    for k, T in enumerate(truth):
        g.add_vertex(T if k == 0 else mul4(T, noise4(rng, st, sr)))
    return g


def _crafted(name):
    rng = np.random.default_rng(sum(map(ord, name)) + SALT.get(name, 0))
    if name == "hub":   # vertex 1 has degree 40: the edge from 0 and 39 to the leaves 2 .. 40, which form a ring
        truth = [path_pose(4 * k) for k in range(41)]
        g = _scattered(rng, truth)
        g.add_edge(0, 1, measure(rng, truth[0], truth[1], 0.002, 0.0006), info(rng))
        for k in range(2, 41):
            g.add_edge(1, k, measure(rng, truth[1], truth[k], 0.002, 0.0006), info(rng))
        for k in range(2, 41):
            nxt = k + 1 if k < 40 else 2
            g.add_edge(k, nxt, measure(rng, truth[k], truth[nxt], 0.01, 0.003), info(rng))
        return g, truth
    if name == "duplicates":   # a dense and a PbMap edge between one pair, as the reference adds them
        truth = [path_pose(32 * k) for k in range(9)]
        g = _chain(rng, truth, [(0, 4), (0, 8)])
        for (i, j) in [(3, 4), (0, 4), (3, 4)]:
            g.add_edge(i, j, measure(rng, truth[i], truth[j], 0.01, 0.003), info(rng))
        return g, truth
    if name == "reversed":   # every other edge given as (j, i)
        truth = [path_pose(32 * k) for k in range(9)]
        g = _chain(rng, truth, [(0, 4), (0, 8), (2, 6)])
        E = []
        for k, (i, j, Z, Om) in enumerate(g.edges):
            E.append((j, i, measure(rng, truth[j], truth[i], 0.002, 0.0006), Om) if k % 2 else (i, j, Z, Om))
        g.edges = E
        return g, truth
    if name == "fixed8":
        truth = [path_pose(4 * k) for k in range(65)]
        return _chain(rng, truth, [(0, 32), (0, 64), (16, 48)], fixed=set(range(4, 65, 8))), truth
    if name == "exact_chain":
        truth = [path_pose(32 * k) for k in range(9)]
        g = M.Graph()
        for T in truth:
            g.add_vertex(T)
        for k in range(8):
            g.add_edge(k, k + 1, M.rel4(truth[k], truth[k + 1]), info(rng))
        g.add_edge(0, 8, M.rel4(truth[0], truth[8]), info(rng))
        return g, truth
    if name == "big_rotations":   # relative rotations of 1.5 .. 2.5 rad along the chain
        truth = [path_pose(0)]
        for k in range(8):
            ax = rng.normal(0, 1, 3)
            step = np.eye(4)
            step[:3, :3] = M.exp_so3(ax / np.linalg.norm(ax) * rng.uniform(1.5, 2.5))
            step[:3, 3] = rng.normal(0, 1.0, 3)
            truth.append(mul4(truth[-1], step))
        g = _scattered(rng, truth, 0.05, 0.05)
        for k in range(8):
            g.add_edge(k, k + 1, measure(rng, truth[k], truth[k + 1], 0.01, 0.003), info(rng))
        for (i, j) in [(0, 4), (0, 8), (2, 6)]:
            g.add_edge(i, j, measure(rng, truth[i], truth[j], 0.002, 0.0006), info(rng))
        return g, truth
    if name == "small_angles":   # residual rotations of exactly zero and of 1e-5 rad beside an ordinary edge
        truth = [path_pose(8 * k) for k in range(3)]
        g = M.Graph()
        for T in truth:
            g.add_vertex(T)
        Z = M.rel4(truth[0], truth[1])
        Z[:3, 3] += [0.01, -0.02, 0.005]
        g.add_edge(0, 1, Z, info(rng))
        tilt = np.eye(4)
        tilt[:3, :3] = M.exp_so3([1e-5, 0.0, 0.0])
        tilt[:3, 3] = [0.0, 0.003, 0.0]
        g.add_edge(1, 2, mul4(M.rel4(truth[1], truth[2]), tilt), info(rng))
        g.add_edge(0, 2, measure(rng, truth[0], truth[2], 0.01, 0.003), info(rng))
        return g, truth
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def get(name):
    g, truth = _sized(int(name[1:])) if name[0] == "n" and name[1:].isdigit() else _crafted(name)
    return Case(name, g, truth)


def random_edges(count, seed=7, max_angle=2.5):
    """(T_i, T_j, Z) triples whose residual rotations reach max_angle (the Jacobian test)."""
    rng = np.random.default_rng(seed)
    out = []

    def rand_pose(amax):
        ax = rng.normal(0, 1, 3)
        T = np.eye(4)
        T[:3, :3] = M.exp_so3(ax / np.linalg.norm(ax) * rng.uniform(0, amax))
        T[:3, 3] = rng.normal(0, 2.0, 3)
        return T
    for _ in range(count):
        Ti, Tj = rand_pose(3.0), rand_pose(3.0)
        out.append((Ti, Tj, mul4(M.rel4(Ti, Tj), rand_pose(max_angle))))
    return out
