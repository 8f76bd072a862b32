"""An independent float64 numpy statement of the PbMap matching stage (RegisterRGBD360::RegisterPbMap,
DESIGN.md §PbMap): subgraph selection, every unary and binary comparison with its verdict and its margin, and the
ConsistencyTest pose by numpy.linalg.svd.  It shares no code with the library (host/pbmap.cpp, kernels/plane_match.hip)
or with the oracle (oracle/src/pbmap_oracle.cpp); the interpretation tree is not restated here (tests/test_match_tree.py
has its exhaustive enumeration).

Planes are dicts with float32 descriptors (normal, center, d, area, elongation, curvature, nrgb, intensity); a plane's
id is its position in the list.  Everything below is evaluated in float64 from those float32 values.

Margins and the bound
---------------------
Every comparison is "reject if x > thr" (or "x < thr").  Its margin is |x - thr| in the comparison's own units.  The
float32 code evaluates x (and sometimes thr) with rounding; an entry is *decided* when every comparison that determines
it has margin > SAFETY * E, E the worst-case float32 evaluation error of that comparison, SAFETY = 16.  E is derived
here, not measured; u = 2^-24 is the float32 unit roundoff, inputs are exact float32 values, and the standard model
fl(a op b) = (a op b)(1 + d), |d| <= u holds for every operation (sqrtf included; no contraction is assumed, and a fused
multiply-add only removes a rounding).  Per comparison:

  area, elongation   x = s, thr = c * t           one product:            E = u c t
  colour, intensity  x = |s - t|                  one difference:         E = u |s - t|
  dist_d             x = |s.d - t.d|              one difference:         E = u |s.d - t.d|
  vertical normal    x = |s.nx - t.nx|            one difference:         E = u |s.nx - t.nx|      (<= 2u)
  |s.nx| gate        x = |s.nx|                   no arithmetic:          E = 0
  unary angle        x = ns . nt                  three products, two sums: |err| <= 3u sum|a_k b_k| <= 3u |ns||nt|;
                                                  float32 unit normals have |n| <= 1 + 2u:   E = 4u
  parallel gate      x = |a|, a = n1 . n2         the same dot product:   E = 4u
  relative angle     x = a b + sa sb, sa = sqrt(max(0, 1 - a^2)) (cos of the difference of the two angles)
      a and b carry 4u each.  1 - a^2 carries 2|a| 4u + u a^2 + u |1 - a^2| <= 8u =: ex absolute, and
      |sqrt(x') - sqrt(x)| = |x' - x| / (sqrt(x') + sqrt(x)) <= min(sqrt(ex), ex / sa) =: esa (+ u sa for sqrtf's own
      rounding).  There is no uniform bound that is useful: next to a = +-1 the square root turns 8u into 7e-4, so E
      depends on the pair:
          E = 4u (|a| + |b|) + 16 u^2 + esa sb + esb sa + esa esb + u (sa + sb) + 3u
      (the last term: two products and one sum of values <= 1).  For sa, sb >= 0.1 this is < 3e-6.
  distance ratio     x = ds2, thr = r2 dt2, ds2 = |c1 - c2|^2
      each difference carries u |ds_k|; squared 2u + u; summed over three non-negative terms 2u more: ds2 is within
      6u ds2 (relative, no cancellation after the differences because all terms are >= 0).  r2 = thr^2 carries u and
      the product r2 dt2 one more:                                        E = u (6 ds2 + 8 r2 dt2)
      For coordinates up to 10 m, ds2 <= 1200 m^2: E <= 14 u 1200 = 1.0e-3 m^2, i.e. 8.3e-7 relative.
  relative height    x = |hs - ht|, hs = n1 . (c2 - c1)
      the differences carry u |es_k|, the dot product 3u sum|n_k es_k| on top:  e_hs = 4u sum|n_k||es_k|; the final
      difference u |hs - ht|.  This is where cancellation lives (hs and ht are nearly equal for a true match), which is
      why E is absolute:                                                  E = e_hs + e_ht + u |hs - ht|
      For coordinates up to 10 m, sum|n_k||es_k| <= |es| (1 + 2u) <= 34.7 m: E <= 1.7e-5 m.

A comparison against a NaN quantity is false in IEEE arithmetic whatever the rounding, so it is decided (margin inf).
An entry is decided-false when some comparison rejects decidedly (for the gated ones: the gate is decidedly on too),
decided-true when every comparison passes decidedly (a gated one: passes decidedly, or its gate is decidedly off).
"""
import numpy as np

U = 2.0 ** -24
SAFETY = 16.0
PI = 3.14159265359                  # include/Miscellaneous.h:44, the constant the thresholds' angles are converted with
MAX_CURVATURE = float(np.float32(0.0013))   # include/Miscellaneous.h:54
CONDITIONING = 8000.0               # threshold_conditioning, include/Miscellaneous.h:76
RANK2 = 1e-6                        # second singular value of M relative to the first

UNARY_NAMES = ("area_s", "area_t", "elong_s", "elong_t", "color0", "color1", "color2", "intensity", "normal_x",
               "dist_d_gated", "angle", "dist_d")
BINARY_NAMES = ("angle", "ratio_s", "ratio_t", "height")


def thresholds(p) -> dict:
    """Float64 values of the float32 thresholds the comparisons use; p has the ini keys as attributes (degrees)."""
    f = lambda v: float(np.float32(v))  # noqa: E731
    return dict(dist_d=f(p.dist_d), cos_unary=f(np.float32(np.cos(f(p.angle) * PI / 180))), color=f(p.color_threshold),
                intensity=f(p.intensity_threshold), elongation=f(p.elongation_threshold), area=f(p.area_threshold),
                dist=f(p.dist_threshold), cos_binary=f(np.float32(np.cos(f(p.angle_threshold) * PI / 180))),
                height=f(p.height_threshold), cos_parallel=f(p.cos_angle_parallel),
                normal_tol=f(np.float32(np.sin(f(p.planar_normal_angle) * PI / 180))))


def select(planes, max_match_planes: int) -> list:
    """setReference / setTarget: planes flatter than MAX_CURVATURE; with a limit below the map's size, those whose area
    strictly exceeds the (P - limit)-th smallest of the areas (curved planes counting as area 0)."""
    P = len(planes)
    flat = np.array([np.float32(p["curvature"]) < np.float32(MAX_CURVATURE) for p in planes], bool)
    if max_match_planes <= 0 or P <= max_match_planes:
        return [i for i in range(P) if flat[i]]
    area = np.where(flat, np.array([np.float32(p["area"]) for p in planes], np.float32), np.float32(0))
    cut = np.sort(area)[P - max_match_planes - 1]
    return [i for i in range(P) if area[i] > cut]


def _arr(planes, ids):
    g = lambda k: np.array([np.asarray(planes[i][k], np.float32) for i in ids], np.float32).astype(np.float64)  # noqa
    return dict(n=g("normal").reshape(-1, 3), c=g("center").reshape(-1, 3), d=g("d"), area=g("area"),
                elong=g("elongation"), rgb=g("nrgb").reshape(-1, 3), inten=g("intensity"))


class Cmp:
    """One comparison over an array of entries: reject, margin, bound E (same shape)."""

    def __init__(self, x, thr, E, less=False):
        with np.errstate(invalid="ignore"):
            x, thr, E = np.broadcast_arrays(np.asarray(x, float), np.asarray(thr, float), np.asarray(E, float))
            self.reject = (x < thr) if less else (x > thr)
            nan = np.isnan(x) | np.isnan(thr)
            self.margin = np.where(nan, np.inf, np.abs(x - thr))
            self.E = np.where(nan, 0.0, E)
            sure = (self.margin > SAFETY * self.E) | (self.E == 0)
        self.sure_reject = self.reject & sure
        self.sure_pass = ~self.reject & sure


def unary(S, T, mode: int, c: dict) -> dict:
    """S, T: _arr() of the selected planes.  -> name -> Cmp over [ns, nt], plus 'ok' and 'decided'."""
    s = {k: v[:, None] for k, v in S.items() if v.ndim == 1}
    t = {k: v[None, :] for k, v in T.items() if v.ndim == 1}
    out = {}
    out["area_s"] = Cmp(s["area"], c["area"] * t["area"], U * np.abs(c["area"] * t["area"]))
    out["area_t"] = Cmp(t["area"], c["area"] * s["area"], U * np.abs(c["area"] * s["area"]))
    out["elong_s"] = Cmp(s["elong"], c["elongation"] * t["elong"], U * np.abs(c["elongation"] * t["elong"]))
    out["elong_t"] = Cmp(t["elong"], c["elongation"] * s["elong"], U * np.abs(c["elongation"] * s["elong"]))
    for k in range(3):
        dk = np.abs(S["rgb"][:, None, k] - T["rgb"][None, :, k])
        out[f"color{k}"] = Cmp(dk, c["color"], U * dk)
    di = np.abs(s["inten"] - t["inten"])
    out["intensity"] = Cmp(di, c["intensity"], U * di)
    dd = np.abs(s["d"] - t["d"])
    names = ["area_s", "area_t", "elong_s", "elong_t", "color0", "color1", "color2", "intensity"]
    shape = dd.shape
    sure_false = np.zeros(shape, bool)
    sure_true = np.ones(shape, bool)
    ok = np.ones(shape, bool)
    if mode in (1, 3):
        dn = np.abs(S["n"][:, None, 0] - T["n"][None, :, 0])
        out["normal_x"] = Cmp(dn, c["normal_tol"], U * dn)
        names.append("normal_x")
        gate = Cmp(np.abs(S["n"][:, None, 0]), c["cos_parallel"], 0.0)
        gated = Cmp(dd, c["dist_d"], U * dd)
        out["gate_x"], out["dist_d_gated"] = gate, gated
        ok &= ~(gate.reject & gated.reject)
        sure_false |= gate.sure_reject & gated.sure_reject
        sure_true &= gate.sure_pass | gated.sure_pass
    if mode in (2, 3):
        dot = (S["n"][:, None, :] * T["n"][None, :, :]).sum(-1)
        out["angle"] = Cmp(dot, c["cos_unary"], 4 * U, less=True)
        out["dist_d"] = Cmp(dd, c["dist_d"], U * dd)
        names += ["angle", "dist_d"]
    for k in names:
        ok &= ~out[k].reject
        sure_false |= out[k].sure_reject
        sure_true &= out[k].sure_pass
    out["ok"] = ok
    out["decided"] = sure_false | sure_true
    return out


def _pairs(A):
    """Per ordered pair (1, 2) of one map's planes: a = n1.n2, sa and its error, |c1 - c2|^2, h = n1.(c2 - c1) and
    its error."""
    n, c = A["n"], A["c"]
    a = n @ n.T
    x = np.fmax(0.0, 1.0 - a * a)
    sa = np.sqrt(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        esa = np.fmin(np.sqrt(8 * U), np.where(sa > 0, 8 * U / sa, np.inf)) + U * sa
    e = c[None, :, :] - c[:, None, :]                     # e[1, 2] = c2 - c1
    d2 = (e * e).sum(-1)
    h = (n[:, None, :] * e).sum(-1)
    eh = 4 * U * (np.abs(n[:, None, :]) * np.abs(e)).sum(-1)
    return dict(a=a, sa=sa, esa=esa, d2=d2, h=h, eh=eh)


def binary_rows(PS, PT, i, c: dict) -> dict:
    """Comparisons of the entries (i, j, k, l) for one reference plane i: Cmp over [nt, ns, nt] (j, k, l)."""
    sp = lambda k: PS[k][i][None, :, None]        # noqa: E731   (i, k) -> broadcast over j, l
    tp = lambda k: PT[k][:, None, :]              # noqa: E731   (j, l) -> broadcast over k
    a, b, sa, sb, esa, esb = sp("a"), tp("a"), sp("sa"), tp("sa"), sp("esa"), tp("esa")
    with np.errstate(invalid="ignore"):
        q = a * b + sa * sb
        Eq = 4 * U * (np.abs(a) + np.abs(b)) + 16 * U * U + esa * sb + esb * sa + esa * esb + U * (sa + sb) + 3 * U
        out = {"angle": Cmp(q, c["cos_binary"], Eq, less=True)}
        r2 = c["dist"] * c["dist"]
        ds2, dt2 = sp("d2"), tp("d2")
        out["ratio_s"] = Cmp(ds2, r2 * dt2, U * (6 * ds2 + 8 * r2 * dt2))
        out["ratio_t"] = Cmp(dt2, r2 * ds2, U * (6 * dt2 + 8 * r2 * ds2))
        gate = Cmp(np.abs(a), c["cos_parallel"], 4 * U)
        dh = np.abs(sp("h") - tp("h"))
        out["height"] = Cmp(dh, c["height"], sp("eh") + tp("eh") + U * dh)
    out["gate"] = gate
    ok = ~out["angle"].reject & ~out["ratio_s"].reject & ~out["ratio_t"].reject & ~(gate.reject & out["height"].reject)
    sure_false = (out["angle"].sure_reject | out["ratio_s"].sure_reject | out["ratio_t"].sure_reject
                  | (gate.sure_reject & out["height"].sure_reject))
    sure_true = (out["angle"].sure_pass & out["ratio_s"].sure_pass & out["ratio_t"].sure_pass
                 & (gate.sure_pass | out["height"].sure_pass))
    nt, ns = PT["a"].shape[0], PS["a"].shape[0]
    distinct = (np.arange(ns)[None, :, None] != i) & (np.arange(nt)[:, None, None] != np.arange(nt)[None, None, :])
    out["ok"] = ok & distinct                       # an assignment is never paired with one sharing a plane
    out["decided"] = sure_false | sure_true | ~distinct
    return out


def pack(ok4) -> np.ndarray:
    """[ns, nt, ns, nt] bool -> the library's layout: [(i * nt + j)][words] uint64, bit k * nt + l."""
    ns, nt = ok4.shape[:2]
    n = ns * nt
    words = (n + 63) // 64
    bits = np.zeros((n, words * 64), np.uint8)
    bits[:, :n] = ok4.reshape(n, n)
    by = np.packbits(bits, axis=-1, bitorder="little")
    return np.ascontiguousarray(by).view("<u8").reshape(n, words).astype(np.uint64)


def unpack(binary, ns, nt) -> np.ndarray:
    n = ns * nt
    by = np.ascontiguousarray(binary.astype("<u8")).view(np.uint8).reshape(n, -1, 8)
    bits = np.unpackbits(by, axis=-1, bitorder="little").reshape(n, -1)
    return bits[:, :n].reshape(ns, nt, ns, nt).astype(bool), bits[:, n:]


def tables(ref, trg, max_match_planes: int, mode: int, params, detail: bool = False, binary_of: dict = None) -> dict:
    """sid, tid, unary [ns, nt] and ok [ns, nt, ns, nt] verdicts with their `decided` masks; detail=True also keeps
    every comparison (name -> Cmp, binary ones per reference plane i).  The binary table does not depend on the mode:
    binary_of = an earlier result for the same maps and thresholds whose binary part is taken over."""
    c = thresholds(params)
    sid, tid = select(ref, max_match_planes), select(trg, max_match_planes)
    S, T = _arr(ref, sid), _arr(trg, tid)
    ns, nt = len(sid), len(tid)
    un = unary(S, T, mode, c)
    PS, PT = _pairs(S), _pairs(T)
    ok4 = np.zeros((ns, nt, ns, nt), bool)
    dec4 = np.ones((ns, nt, ns, nt), bool)
    rows = []
    if binary_of is not None:
        ok4, dec4, rows = binary_of["ok"], binary_of["decided"], binary_of.get("binary_cmp", [])
    for i in range(ns if binary_of is None else 0):
        r = binary_rows(PS, PT, i, c)
        ok4[i], dec4[i] = r["ok"], r["decided"]
        if detail:
            rows.append(r)
    out = dict(sid=np.array(sid, np.int32), tid=np.array(tid, np.int32), unary=un["ok"].astype(np.uint8),
               unary_decided=un["decided"], ok=ok4, decided=dec4)
    if detail:
        out["unary_cmp"] = {k: v for k, v in un.items() if isinstance(v, Cmp)}
        out["binary_cmp"] = rows
    return out


def agree(model: dict, got: dict) -> list:
    """Differences between the model's decided entries and a {sid, tid, unary, binary} table set."""
    bad = []
    if not (np.array_equal(model["sid"], got["sid"]) and np.array_equal(model["tid"], got["tid"])):
        return ["selection"]
    ns, nt = len(model["sid"]), len(model["tid"])
    if ns == 0 or nt == 0:
        return bad
    du = (model["unary"] != got["unary"].reshape(ns, nt)) & model["unary_decided"]
    bad += [("unary",) + tuple(int(v) for v in ix) for ix in np.argwhere(du)[:8]]
    ok4, pad = unpack(got["binary"], ns, nt)
    db = (model["ok"] != ok4) & model["decided"]
    bad += [("binary",) + tuple(int(v) for v in ix) for ix in np.argwhere(db)[:8]]
    if pad.any():
        bad.append("padding bits set")
    return bad


def undecided(model: dict):
    """(undecided entries, entries) over the unary and binary tables."""
    return (int((~model["unary_decided"]).sum() + (~model["decided"]).sum()),
            int(model["unary_decided"].size + model["decided"].size))


# ------------------------------------------------------------------------------------------------ pose
def pose(ref, trg, matches: dict):
    """ConsistencyTest::estimatePoseWithCovariance: (ok, P [4, 4] with x_ref = P x_trg, information [6, 6]).
    Rotation: Kabsch on the target-area-weighted normals by SVD with the determinant correction; translation: the
    pseudo-inverse solution of sum w nr nr^T t = sum w nr (d_t - d_r); false with fewer than three matches, with
    fewer than two independent normals, or when sum w nr nr^T is worse conditioned than CONDITIONING."""
    if len(matches) < 3:
        return False, None, None
    M, Ht, Hr, g = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(3)
    for r, t in sorted(matches.items()):
        nr = np.asarray(ref[r]["normal"], np.float32).astype(float)
        nt = np.asarray(trg[t]["normal"], np.float32).astype(float)
        w = float(np.float32(trg[t]["area"]))
        M += w * np.outer(nt, nr)
        Ht += w * np.outer(nr, nr)
        Hr += w * (np.eye(3) - np.outer(nr, nr))
        g += w * nr * (float(np.float32(trg[t]["d"])) - float(np.float32(ref[r]["d"])))
    if not (np.isfinite(M).all() and np.isfinite(g).all()):
        return False, None, None                       # every comparison on NaN singular values is false
    Um, sig, Vh = np.linalg.svd(M)
    if not sig[1] > RANK2 * sig[0]:
        return False, None, None
    Rm = Vh.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(Vh.T @ Um.T))]) @ Um.T
    lt = np.linalg.eigvalsh(Ht)[::-1]
    if not lt[2] > 0 or lt[0] / lt[2] > CONDITIONING:
        return False, None, None
    P = np.eye(4)
    P[:3, :3] = Rm
    P[:3, 3] = np.linalg.pinv(Ht) @ g
    info = np.zeros((6, 6))
    info[:3, :3], info[3:, 3:] = Ht, Hr
    return True, P, info


def pose_drift(P, G):
    """(rotation angle of P G^-1 in rad, |t_P - t_G| in m)."""
    Rd = np.asarray(P, float)[:3, :3] @ np.asarray(G, float)[:3, :3].T
    s = 0.5 * np.linalg.norm([Rd[2, 1] - Rd[1, 2], Rd[0, 2] - Rd[2, 0], Rd[1, 0] - Rd[0, 1]])
    return float(np.arctan2(s, (np.trace(Rd) - 1) / 2)), float(np.linalg.norm(np.asarray(P, float)[:3, 3] -
                                                                              np.asarray(G, float)[:3, 3]))
