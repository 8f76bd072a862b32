"""Crafted plane maps for the PbMap matcher and pose tests (tests/test_match_model.py on the CPU,
tests/test_gpu_match_shapes.py on the GPU).  Everything is deterministic; a plane is a dict of float32 descriptors and
its id is its position in its map.  A case is a dict: name, ref, trg (lists of planes), mmp (max_match_planes), modes
(registration types that read what the case is about), kind ("random": planes drawn by scene(), whatever is then
done to them; "crafted": every plane placed by hand around one threshold; "exact": a quantity on its threshold), and
where known: G (x_ref = G x_trg) and truth (ref id -> trg id of the construction).

The target map of a scene is the reference map moved by G = (R, t): n_t = R^T n_r, c_t = R^T (c_r - t),
d_t = d_r + n_r . t, computed in float64 and rounded once.
"""
import os

import numpy as np

from oracle import oracle360 as O

CONFIG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "config_files")
INIS = (None, "configLocaliser_spherical.ini")          # the default thresholds and the relocalisation file's
EPS = 2.0 ** -10                                         # threshold cases sit at thr (1 -+ EPS)


def params(ini):
    return O.load_match_ini(os.path.join(CONFIG_DIR, ini)) if ini else O.MatchParams.odometry_default()


def f32(v):
    return np.asarray(v, np.float64).astype(np.float32)


def plane(n, c, d=None, area=2.0, elong=2.0, rgb=(0.3, 0.3, 0.3), inten=100.0, curv=0.0):
    n, c = np.asarray(n, np.float64), np.asarray(c, np.float64)
    return dict(normal=f32(n), center=f32(c), d=np.float32(-(n @ c) if d is None else d), area=np.float32(area),
                elongation=np.float32(elong), curvature=np.float32(curv), nrgb=f32(rgb), intensity=np.float32(inten),
                ppal=f32((0, 0, 0)), sensor=0, n_inliers=1,
                hull=f32([c, c, c, c]))            # a minimal 4-point hull: the matcher never reads it


def copy(p, **kw):
    q = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    for k, v in kw.items():
        q[k] = f32(v) if np.ndim(v) else (np.float32(v) if k not in ("sensor", "n_inliers") else v)
    return q


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def rigid(axis, deg, t):
    G = np.eye(4)
    G[:3, :3] = rot(axis, deg)
    G[:3, 3] = t
    return G


def moved(p, G):
    """The plane p of the reference map as the target map sees it (x_ref = G x_trg)."""
    R, t = G[:3, :3], G[:3, 3]
    n, c = p["normal"].astype(np.float64), p["center"].astype(np.float64)
    return copy(p, normal=R.T @ n, center=R.T @ (c - t), d=float(p["d"]) + n @ t, hull=[R.T @ (c - t)] * 4)


def random_plane(rng, normal=None):
    n = rng.normal(size=3) if normal is None else np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    # log-uniform areas over three decades, elongations over [1, 6], colours over a range nine thresholds wide:
    # two unrelated planes pass the unary tests with probability of about 1 %
    return plane(n, rng.uniform(-5, 5, 3), area=float(np.exp(rng.uniform(np.log(0.15), np.log(150)))),
                 elong=rng.uniform(1, 6), rgb=rng.uniform(0.05, 0.65, 3), inten=rng.uniform(0, 255))


def scene(seed, ns, nt, G=None, common=None):
    """ns reference and nt target planes sharing `common` planes (moved by G, in permuted positions); the others are
    distractors on either side.  The first three common normals are an orthonormal frame (a guaranteed spread)."""
    rng = np.random.default_rng(seed)
    if G is None:
        G = rigid(rng.normal(size=3), rng.uniform(2, 25), rng.uniform(-0.5, 0.5, 3))
    if common is None:
        common = min(ns, nt) - (2 if min(ns, nt) >= 7 else 0)
    frame = rot(rng.normal(size=3), rng.uniform(0, 180))
    shared = [random_plane(rng, frame[:, k] if k < 3 else None) for k in range(common)]
    ref = shared + [random_plane(rng) for _ in range(ns - common)]
    trg = [moved(p, G) for p in shared] + [random_plane(rng) for _ in range(nt - common)]
    pr, pt = rng.permutation(ns), rng.permutation(nt)     # new position -> old position
    ref, trg = [ref[k] for k in pr], [trg[k] for k in pt]
    where_r, where_t = np.argsort(pr), np.argsort(pt)
    truth = {int(where_r[k]): int(where_t[k]) for k in range(common)}
    return dict(name=f"scene{ns}x{nt}s{seed}", ref=ref, trg=trg, mmp=0, modes=(0, 1, 2, 3), G=G, truth=truth,
                kind="random")


# table shapes: ns * nt of 63 / 64 / 65 (7x9, 8x8, 5x13 and 13x5), exactly two words (64x2: 128 pairs), lopsided
# maps, more than 64 targets (70x66: the interpretation tree's multi-word domains), listed large before small so that
# a context that has grown its tables serves the small ones after
SHAPES = ((70, 66), (1, 1), (33, 31), (2, 3), (64, 2), (3, 3), (40, 3), (7, 9), (3, 40), (8, 8), (25, 25), (5, 13),
          (13, 5))


def shape_cases():
    return [scene(100 + k, ns, nt) for k, (ns, nt) in enumerate(SHAPES)]


# ------------------------------------------------------------------------------------------------ thresholds
def _base():
    """Two planes seen twice (G = identity): every comparison passes with a wide margin in every mode."""
    p0 = plane((0, 1, 0), (0, 2, 0), area=2.0, elong=2.0, inten=160.0)
    p1 = plane((0, 0, 1), (3, 1, 3), area=3.0, elong=2.6, rgb=(0.32, 0.3, 0.28), inten=170.0)
    return [p0, p1], [copy(p0), copy(p1)]


def _pair(name, modes, make, entry):
    """make(side) -> (ref, trg) with the quantity at thr (1 + side EPS); entry: the table entry it is aimed at."""
    lo, hi = make(-1.0), make(+1.0)
    mk = lambda s, rt: dict(name=f"{name}{s}", ref=rt[0], trg=rt[1], mmp=0, modes=modes, kind="crafted")   # noqa
    return dict(name=name, modes=modes, below=mk("-", lo), above=mk("+", hi), entry=entry)


def threshold_cases(ini):
    """Every unary and binary comparison at thr (1 -+ 2^-10) (additive thresholds: thr -+ thr 2^-10), for one threshold
    set.  entry = ("unary", i, j) or ("binary", i, j, k, l); `cmp` names the comparison in match_model's tables;
    `modes`: the registration types in which the entry must flip between the two maps."""
    from match_model import thresholds
    c = thresholds(params(ini))
    out = []

    def add(name, modes, cmp, entry, make, same=()):
        d = _pair(name, modes, make, entry)
        d["cmp"], d["same"] = cmp, same          # same: modes in which the two maps must give one table
        out.append(d)

    def vary_trg0(**kw_of_side):
        def make(side):
            ref, trg = _base()
            trg[0] = copy(trg[0], **{k: v(side) for k, v in kw_of_side.items()})
            return ref, trg
        return make

    e = lambda side: 1.0 + side * EPS   # noqa: E731
    allm = (0, 1, 2, 3)
    # the two-sided ratio tests, each side on its own
    add("area_t", allm, "area_t", ("unary", 0, 0), vary_trg0(area=lambda s: 2.0 * c["area"] * e(s)))
    add("area_s", allm, "area_s", ("unary", 0, 0), vary_trg0(area=lambda s: 2.0 / (c["area"] * e(s))))
    add("elong_t", allm, "elong_t", ("unary", 0, 0), vary_trg0(elongation=lambda s: 2.0 * c["elongation"] * e(s)))
    add("elong_s", allm, "elong_s", ("unary", 0, 0), vary_trg0(elongation=lambda s: 2.0 / (c["elongation"] * e(s))))
    for k in range(3):
        for sign in (+1, -1):
            def rgb(s, k=k, sign=sign):
                v = [0.3, 0.3, 0.3]
                v[k] += sign * c["color"] * e(s)
                return v
            add(f"color{k}{'+' if sign > 0 else '-'}", allm, f"color{k}", ("unary", 0, 0), vary_trg0(nrgb=rgb))
    add("intensity+", allm, "intensity", ("unary", 0, 0), vary_trg0(intensity=lambda s: 160.0 + c["intensity"] * e(s)))
    add("intensity-", allm, "intensity", ("unary", 0, 0), vary_trg0(intensity=lambda s: 160.0 - c["intensity"] * e(s)))

    # modes 1 and 3: the vertical (x) component of the normal within sin(10 deg), from either side
    for sign in (+1, -1):
        def make(side, sign=sign):
            ref, trg = _base()
            nx = 0.3 + sign * c["normal_tol"] * e(side)
            ref[0] = copy(ref[0], normal=(0.3, np.sqrt(1 - 0.09), 0))
            trg[0] = copy(trg[0], normal=(nx, np.sqrt(1 - nx * nx), 0))
            return ref, trg
        add(f"normal_x{'+' if sign > 0 else '-'}", (1, 3), "normal_x", ("unary", 0, 0), make)

    # modes 1 and 3: |n_x| > cos_angle_parallel switches the offset test on; the offsets differ by 2 dist_d.  In mode
    # 3 the same offset test also runs ungated, so there the two maps give the same (rejecting) tables.
    for sign in (+1, -1):
        def make(side, sign=sign):
            ref, trg = _base()
            g = sign * c["cos_parallel"] * e(side)
            n = (g, np.sqrt(1 - g * g), 0)
            ref[0] = copy(ref[0], normal=n)
            trg[0] = copy(trg[0], normal=n, d=float(ref[0]["d"]) + 2 * c["dist_d"])
            return ref, trg
        add(f"gate_x{'+' if sign > 0 else '-'}", (1,), "gate_x", ("unary", 0, 0), make, same=(0, 2, 3))

    # dist_d: behind the gate (a horizontal plane, n = x: mode 1; modes 2 and 3 read it ungated) and on a vertical
    # plane (modes 2 and 3 only; mode 1 must not read it)
    for nm, n0 in (("h", (1, 0, 0)), ("v", (0, 1, 0))):
        for sign in (+1, -1):
            def make(side, sign=sign, n0=n0):
                ref, trg = _base()
                ref[0] = copy(ref[0], normal=n0)
                trg[0] = copy(trg[0], normal=n0, d=float(ref[0]["d"]) + sign * c["dist_d"] * e(side))
                return ref, trg
            add(f"dist_d_{nm}{'+' if sign > 0 else '-'}", (1, 2, 3) if nm == "h" else (2, 3), "dist_d",
                ("unary", 0, 0), make, same=(0,) if nm == "h" else (0, 1))

    # modes 2 and 3: the normals within `angle`; rotated about x so that mode 3's n_x test stays satisfied, and with
    # the second plane's normal along x so that the pair's relative angle is unchanged
    def make(side):
        ref, trg = _base()
        cs = c["cos_unary"] * e(-side)                       # side +1: beyond the angle, cos below the threshold
        ref[1] = copy(ref[1], normal=(1, 0, 0), d=-3.0)
        trg[1] = copy(trg[1], normal=(1, 0, 0), d=-3.0)
        trg[0] = copy(trg[0], normal=(0, cs, np.sqrt(1 - cs * cs)))
        return ref, trg
    add("angle", (2, 3), "angle", ("unary", 0, 0), make)

    # ---- binary (every mode builds the same binary table)
    # relative angle: the reference pair at 60 deg, the target pair at 60 +- the threshold
    for sign in (+1, -1):
        def make(side, sign=sign):
            ref, trg = _base()
            dlt = np.arccos(c["cos_binary"] * e(-side))
            ref[1] = copy(ref[1], normal=(0, np.cos(np.pi / 3), np.sin(np.pi / 3)))
            a = np.pi / 3 + sign * dlt
            trg[1] = copy(trg[1], normal=(0, np.cos(a), np.sin(a)))
            return ref, trg
        add(f"rel_angle{'+' if sign > 0 else '-'}", allm, "angle", ("binary", 0, 0, 1, 1), make)

    # centroid-distance ratio, each side on its own: the reference centres 2 m apart, the target ones 2 thr or 2 / thr
    for nm, inv in (("ratio_t", False), ("ratio_s", True)):
        def make(side, inv=inv):
            ref, trg = _base()
            L = 2.0 / (c["dist"] * e(side)) if inv else 2.0 * c["dist"] * e(side)
            ref[0] = copy(ref[0], center=(0, 2, 0))
            ref[1] = copy(ref[1], center=(2, 2, 0))
            trg[0] = copy(trg[0], center=(0, 2, 0))
            trg[1] = copy(trg[1], center=(L, 2, 0))
            return ref, trg
        add(nm, allm, nm, ("binary", 0, 0, 1, 1), make)

    # the parallel gate |a| > cos_angle_parallel on both sides, for a > 0 and for a < 0 (anti-parallel planes, floor
    # against ceiling); the relative heights differ by 2 height_threshold
    for sign in (+1, -1):
        def make(side, sign=sign):
            ref, trg = _base()
            g = c["cos_parallel"] * e(side)
            n1 = (0, sign * g, sign * np.sqrt(1 - g * g))
            ref[1] = copy(ref[1], normal=n1, center=(3, 1, 0), d=-3.0)
            trg[1] = copy(trg[1], normal=n1, center=(3, 1 + 2 * c["height"], 0), d=-3.0)
            return ref, trg
        add(f"gate_par{'+' if sign > 0 else '-'}", allm, "gate", ("binary", 0, 0, 1, 1), make)

    # relative height of parallel (a = 1) and anti-parallel (a = -1) planes, up and down
    for sign in (+1, -1):
        for up in (+1, -1):
            def make(side, sign=sign, up=up):
                ref, trg = _base()
                ref[1] = copy(ref[1], normal=(0, sign, 0), center=(3, 1, 0), d=-3.0)
                trg[1] = copy(trg[1], normal=(0, sign, 0), center=(3, 1 + up * c["height"] * e(side), 0), d=-3.0)
                return ref, trg
            add(f"height{'p' if sign > 0 else 'a'}{'+' if up > 0 else '-'}", allm, "height", ("binary", 0, 0, 1, 1),
                make)
    return out


def exact_cases(ini):
    """The tested quantity equals its threshold exactly in float32 (products by a power of two, differences from
    zero, 3-4-5 free axis-aligned distances): `x > thr` is false on both sides whatever the rounding.  Compared with
    the oracle only; the model leaves these entries undecided."""
    p = params(ini)
    out = []

    def add(name, modes, ref, trg):
        out.append(dict(name=f"exact_{name}", ref=ref, trg=trg, mmp=0, modes=modes, kind="exact"))

    thr = {k: float(np.float32(getattr(p, k))) for k in ("area_threshold", "elongation_threshold", "color_threshold",
                                                          "intensity_threshold", "dist_d", "dist_threshold",
                                                          "height_threshold")}
    allm = (0, 1, 2, 3)
    for key, fld, base in (("area_threshold", "area", 2.0), ("elongation_threshold", "elongation", 2.0)):
        ref, trg = _base()
        ref[0] = copy(ref[0], **{fld: base})
        trg[0] = copy(trg[0], **{fld: base * thr[key]})        # 2 thr is exact in float32
        add(fld, allm, ref, trg)
    ref, trg = _base()
    ref[0] = copy(ref[0], nrgb=(0, 0.3, 0.3), intensity=0.0)
    trg[0] = copy(trg[0], nrgb=(thr["color_threshold"], 0.3, 0.3), intensity=thr["intensity_threshold"])
    add("color_intensity", allm, ref, trg)
    ref, trg = _base()
    ref[0] = copy(ref[0], normal=(1, 0, 0), d=0.0)
    trg[0] = copy(trg[0], normal=(1, 0, 0), d=thr["dist_d"])
    add("dist_d", (1, 2, 3), ref, trg)
    ref, trg = _base()
    ref[0], ref[1] = copy(ref[0], center=(0, 0, 0)), copy(ref[1], center=(1, 0, 0))
    trg[0], trg[1] = copy(trg[0], center=(0, 0, 0)), copy(trg[1], center=(thr["dist_threshold"], 0, 0))
    add("ratio", allm, ref, trg)
    ref, trg = _base()
    ref[0], ref[1] = copy(ref[0], center=(0, 0, 0), d=0.0), copy(ref[1], normal=(0, -1, 0), center=(3, 0, 0), d=0.0)
    trg[0] = copy(trg[0], center=(0, 0, 0), d=0.0)
    trg[1] = copy(trg[1], normal=(0, -1, 0), center=(3, thr["height_threshold"], 0), d=0.0)
    add("height", allm, ref, trg)
    return out


def twin_case():
    """Two reference planes (and two target planes) with one centre and one normal: the only way an entry whose two
    assignments share a plane can pass every geometric comparison (distances 0 = 0, heights 0 = 0), so the only thing
    that keeps those entries zero is the table's own k != i, l != j rule."""
    sc = scene(77, 6, 6, common=6)
    ref, trg = sc["ref"], sc["trg"]
    ref[4] = copy(ref[1])
    trg[2] = copy(trg[5])
    return dict(name="twins", ref=ref, trg=trg, mmp=0, modes=(0, 1, 2, 3), kind="random")


# ------------------------------------------------------------------------------------------------ selection
def selection_cases():
    """30 planes under max_match_planes 25, 29, 30, 1 and 0.  Curvature: planes 3 and 17 exactly at the limit 0.0013,
    planes 8 and 22 above it; 8 and 17 are the two largest.  Areas: the three smallest flat planes tie, which is where
    the limit of 25 cuts (the strict comparison then keeps 23); the second and third largest flat planes tie too."""
    sc = scene(55, 30, 30, common=30)
    order = np.random.default_rng(5).permutation(30)
    areas = 1.0 + 0.25 * np.arange(30)                    # distinct multiples of 0.25: exact in float32
    for rank, k in enumerate(order):
        sc["ref"][k] = copy(sc["ref"][k], area=areas[rank])
    big = [int(k) for k in np.argsort([-float(p["area"]) for p in sc["ref"]])]
    curved = {big[0]: 0.0013, big[1]: 0.002}
    small = [k for k in big[::-1]]
    rest = [k for k in range(30) if k not in (big[0], big[1])]
    curved[rest[3]], curved[rest[17]] = 0.0013, 0.0014
    for k, cv in curved.items():
        sc["ref"][k] = copy(sc["ref"][k], curvature=cv)
    flat_small = [k for k in small if k not in curved][:3]
    for k in flat_small:
        sc["ref"][k] = copy(sc["ref"][k], area=1.5)
    flat_big = [k for k in big if k not in curved][:3]
    sc["ref"][flat_big[2]] = copy(sc["ref"][flat_big[2]], area=float(sc["ref"][flat_big[1]]["area"]))
    # the target map: the same planes moved (same areas and curvatures), at their permuted positions
    for r, t in sc["truth"].items():
        sc["trg"][t] = moved(sc["ref"][r], sc["G"])
    return [dict(sc, name=f"select{m}", mmp=m, modes=(0,)) for m in (25, 29, 30, 1, 0)]


# ------------------------------------------------------------------------------------------------ pose
def pose_cases():
    """Mode-0 registrations with a known answer.  expect: True = registers and the pose is G; False = must fail."""
    out = []
    for k, (axis, deg) in enumerate((((1, 0, 0), 0.0), ((1, 2, 3), 5.0), ((0, 1, -1), 90.0), ((-2, 1, 0.5), 170.0))):
        sc = scene(200 + k, 8, 8, G=rigid(axis, deg, (0.3 * k - 0.4, 0.2, -0.25 * k)), common=8)
        out.append(dict(sc, name=f"pose{int(deg)}", modes=(0,), expect=True))
    # mirrored target: a reflection is not a rigid motion; the matcher accepts it in mode 0 (angles, distances and
    # heights are preserved) and the pose estimate goes through the det <= 0 branch
    sc = scene(210, 8, 8, G=np.eye(4), common=8)
    S = np.diag([1.0, 1.0, -1.0])
    for r, t in sc["truth"].items():
        p = sc["ref"][r]
        sc["trg"][t] = copy(p, normal=S @ p["normal"].astype(float), center=S @ p["center"].astype(float))
    out.append(dict(sc, name="mirror", modes=(0,), expect="proper", G=None))

    def fixed_normals(seed, normals, G, name, expect, areas=None):
        rng = np.random.default_rng(seed)
        ref = []
        for k, n in enumerate(normals):
            p = random_plane(rng, n)
            if areas is not None:
                p = copy(p, area=areas[k])
            ref.append(p)
        trg = [moved(p, G) for p in ref]
        return dict(name=name, ref=ref, trg=trg, mmp=0, modes=(0,), G=G, truth={k: k for k in range(len(ref))},
                    expect=expect, kind="random")

    G = rigid((0.2, 1, 0.1), 7.0, (0.2, -0.1, 0.3))
    x, y, z = np.eye(3)
    out.append(fixed_normals(220, [x, -x, y, -y, x, y], G, "corridor", False))      # two directions: no third axis
    out.append(fixed_normals(221, [x, -x, x, -x, x], G, "parallel", False))          # one direction: rank 1
    for nm, side, ok in (("cond-", -1, True), ("cond+", +1, False)):
        # three orthogonal normals: the eigenvalues of sum w nr nr^T are the target areas
        out.append(fixed_normals(222, [x, y, z], G, nm, ok, areas=[8000.0 * (1 + side * 2.0 ** -6), 40.0, 1.0]))
    out.append(dict(scene(223, 2, 2, common=2), name="two", modes=(0,), expect=False))
    # one target plane whose normal and offset are NaN (DESIGN.md §Plane stage: a one-pixel-wide region); it keeps
    # its other descriptors, so the matcher pairs it with its reference plane
    sc = scene(224, 6, 6, common=6)
    t = sc["truth"][2]
    sc["trg"][t] = copy(sc["trg"][t], normal=(np.nan, np.nan, np.nan), d=np.nan)
    out.append(dict(sc, name="nan", modes=(0,), expect=None))
    return out


def all_table_cases():
    """(case, ini, in the exact family) for every case whose tables are compared."""
    out = [(c, ini, False) for ini in INIS for c in shape_cases() + [twin_case()] + selection_cases() + pose_cases()]
    for ini in INIS:
        for th in threshold_cases(ini):
            out += [(th["below"], ini, False), (th["above"], ini, False)]
        out += [(c, ini, True) for c in exact_cases(ini)]
    return out
