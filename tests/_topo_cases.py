"""Inputs of the topological-map tests: the "rooms" graph, the degenerate graphs and the scripted keyframe run."""
import numpy as np

# (n, rooms) of the parity cases: the small sizes, the sizes around 64 / 128 / 256, 100 / 101, and 96 / 97, the two
# sizes on either side of the switch from LDS to the global scratch (R360_TOPO_LDS_MAX_NODES = 96)
SIZES = [(3, 1), (4, 1), (6, 2), (7, 2), (12, 3), (63, 5), (64, 5), (65, 5), (96, 6), (97, 6), (100, 6), (101, 6),
         (128, 8), (129, 8), (255, 12), (256, 12)]
LDS_MAX_NODES = 96
# the seed of each parity case: the first of 1, 2, 3, ... at which every bisection of the recursion satisfies
# topo_model.assert_well_posed (tests/test_topo_model.py checks all of them on the CPU)
SEED = {}


def seed_of(n, rooms):
    return SEED.get((n, rooms), 1)


def rooms_graph(n, rooms, seed):
    """room = sort(randint(0, rooms, n)); for i < j, d = j - i: an edge when d <= 5 or with probability 0.05, of
    weight float32((0.3 + 0.6 u) (1 if same room else 0.08) / (1 + 0.2 d if d <= 5 else 1)); symmetric, zero
    diagonal."""
    rs = np.random.RandomState(seed)
    room = np.sort(rs.randint(0, rooms, n))
    chance = rs.uniform(size=(n, n))
    u = rs.uniform(size=(n, n))
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    d = j - i
    near = d <= 5
    edge = (d > 0) & (near | (chance < 0.05))
    w = (0.3 + 0.6 * u) * np.where(room[i] == room[j], 1.0, 0.08) / np.where(near & (d > 0), 1.0 + 0.2 * d, 1.0)
    A = np.where(edge, w, 0.0).astype(np.float32)
    return A + A.T


def case(n, rooms):
    return rooms_graph(n, rooms, seed_of(n, rooms))


def degenerate(kind, n):
    if kind == "zero":
        return np.zeros((n, n), np.float32)
    if kind == "cliques":   # two disconnected cliques
        A = np.zeros((n, n), np.float32)
        h = n // 2
        A[:h, :h] = 1
        A[h:, h:] = 1
    elif kind == "complete":
        A = np.full((n, n), 0.5, np.float32)
    else:
        raise ValueError(kind)
    np.fill_diagonal(A, 0)
    return A


def scripted_run():
    """The 12-keyframe script of the bookkeeping tests, a list of steps: ("kf",), ("conn", a, b, sso), ("cut",),
    ("drop",).  Three rooms of four keyframes each, strongly tied inside, the second tied to the first by 0.3 of that and the third to the second by 0.03: the first cut
    (after keyframe 11) turns the one area into three; a second cut right after it changes nothing (k <= 0); a
    thirteenth keyframe is added and dropped; then one joins the last area with a connection into the first one, which
    makes those two areas neighbours."""
    steps = []
    for k in range(12):
        steps.append(("kf",))
        for b in range(max(0, k - 3), k):
            tie = 1.0 if b // 4 == k // 4 else (0.3 if k // 4 == 1 else 0.03)
            steps.append(("conn", b, k, (0.9 - 0.1 * (k - b)) * tie))
    steps.append(("cut",))
    steps.append(("cut",))
    steps += [("kf",), ("conn", 11, 12, 0.7), ("drop",)]
    steps += [("kf",), ("conn", 11, 12, 0.8), ("conn", 10, 12, 0.6), ("conn", 1, 12, 0.3), ("cut",)]
    return steps
