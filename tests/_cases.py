"""Shared test inputs and bars (no tests here)."""
import numpy as np


def lambda_family(seed=3):
    """(H + lambda diag H) over alignFrames360's lambda schedule (1, then /5 per accepted update, :4589, :4718)
    for near-singular float Hessians (one direction almost unobserved, as on a textureless or planar level)."""
    rng = np.random.default_rng(seed)
    out = []
    for trial in range(40):
        A = rng.normal(size=(200, 6))
        A[:, 5] = A[:, 0] * rng.normal() + A[:, 1] * rng.normal() + rng.normal(size=200) * 10.0 ** rng.uniform(-6, -2)
        H = (A.T @ A).astype(np.float32)
        lam = 1.0
        for it in range(11):
            M = H.copy()
            for k in range(6):
                M[k, k] = np.float32(H[k, k] + np.float32(np.float32(lam) * H[k, k]))
            out.append((trial, it, M))
            lam /= 5.0
    return out


def icp_check(H, g, e2, nv, nvis, Hr, gr, e2r, nvr, nvisr, npx):
    """The projection is bit-identical (glibc-exact asinf/atan2f port), so pixel sets and counts
    match exactly; the sums differ only by summation order (GPU: per-thread f32 partials over a few
    pixels, then fp64), bounded per component by 1e-5 of the Cauchy-Schwarz scale sqrt(H_kk e2)."""
    assert (nv, nvis) == (nvr, nvisr)
    sH = np.abs(Hr).max()
    assert np.abs(H - Hr).max() <= 1e-5 * sH
    scale = np.sqrt(np.abs(np.diag(Hr)) * max(e2r, 1e-30))
    assert (np.abs(g - gr) <= 1e-5 * scale + 1e-12).all(), (g - gr, scale)
    assert abs(e2 - e2r) <= 1e-6 * e2r


def noise_sphere(rows, cols, seed):
    """BGR uniform; range uniform in [0, 7000) mm with 20 % zeros; a block of the depth bounds' own values (300, 301,
    5999, 6000 mm); a flat patch (harm() = 0: no strict monotony) and a ramp (harm()'s harmonic-mean branch)."""
    rng = np.random.default_rng(seed)
    bgr = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    dep = rng.integers(0, 7000, (rows, cols)).astype(np.uint16)
    dep[rng.random((rows, cols)) < 0.2] = 0
    bounds = np.array([300, 301, 5999, 6000], np.uint16)
    r0, c0 = rows // 2, cols // 2
    hb, wb = min(4, rows - r0), min(8, cols - c0)
    dep[r0:r0 + hb, c0:c0 + wb] = np.resize(bounds, (hb, wb))
    hp, wp = min(12, rows), min(24, cols // 2)
    bgr[:hp, :wp] = 90                      # flat patch
    dep[:hp, :wp] = 2000
    ramp = np.arange(wp, dtype=np.int64)    # monotone ramp, rows shifted so that it rises downwards too
    rr = ramp[None, :] + np.arange(hp)[:, None]
    bgr[rows - hp:, cols - wp:] = (40 + 3 * rr)[..., None].astype(np.uint8)
    dep[rows - hp:, cols - wp:] = (1000 + 25 * rr).astype(np.uint16)
    return bgr, dep


ROOM_HALF = (1.6, 2.4, 3.4)                      # half extents (m) of the box room about the origin
ROOM_TARGET = ((0.1, -0.2, 0.3), 1)              # (eye, seed) of the room pair's target ...
ROOM_SOURCE = ((0.3, 0.0, 0.6), 2)               # ... and source: the source is displaced by (0.2, 0.2, 0.3) m
ROOM_MOTION = tuple(s - t for s, t in zip(ROOM_SOURCE[0], ROOM_TARGET[0]))


def room_sphere(rows, cols, eye, seed, holes=0.1):
    """A textured box room (half extents ROOM_HALF about the origin) seen from `eye` as a rows x cols sphere of the
    library's geometry: the ray through pixel (r, c) has phi = (rows/2 - 0.5 - r) 2 pi / cols, th = c 2 pi / cols - pi
    and direction (sin phi, cos phi sin th, cos phi cos th).  Range to the nearest wall in mm (u16); a smooth texture of
    the hit point, so two eyes see one scene and an alignment converges; `holes` of the pixels, drawn from `seed`, get
    range 0.  Returns (BGR u8 [rows, cols, 3], range u16 [rows, cols])."""
    ares = 2 * np.pi / cols
    phi = (rows / 2 - 0.5 - np.arange(rows)) * ares
    th = np.arange(cols) * ares - np.pi
    d = np.stack([np.sin(phi)[:, None] * np.ones(cols)[None, :],
                  np.cos(phi)[:, None] * np.sin(th)[None, :],
                  np.cos(phi)[:, None] * np.cos(th)[None, :]], axis=-1)
    e = np.asarray(eye, np.float64)
    half = np.asarray(ROOM_HALF, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (half - e) / d, np.where(d < 0, (-half - e) / d, np.inf))
    rng_m = t.min(axis=-1)
    h = e + rng_m[..., None] * d
    hx, hy, hz = h[..., 0], h[..., 1], h[..., 2]
    tex = (128 + 50 * np.sin(3.1 * hx + 1.7 * hy) + 50 * np.cos(2.3 * hz - 1.1 * hy)
           + 20 * np.sin(9 * hx) * np.cos(7 * hz))
    tex = np.rint(np.clip(tex, 0, 255))                                 # the 8-bit texture value t
    bgr = np.stack([tex, 0.8 * tex + 20, 255 - tex], axis=-1).astype(np.uint8)   # 0.8 t + 20 <= 224, truncated
    dep = np.rint(rng_m * 1000.0).astype(np.uint16)
    dep[np.random.default_rng(seed).random((rows, cols)) < holes] = 0
    return bgr, dep


def room_pair(rows, cols):
    """(target images, source images) of the room at rows x cols."""
    return room_sphere(rows, cols, *ROOM_TARGET), room_sphere(rows, cols, *ROOM_SOURCE)


# ------------------------------------------------------------------ plane half: shared comparisons and inputs
def same(a, b):
    """bitwise equality with NaN == NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def per_sensor_oracle(b, dm):
    """The oracle's per-pixel stages and segmentation of the 8 sensors of one frame (BGR images, depth in metres)."""
    from oracle import oracle360 as O
    out = []
    for k in range(8):
        xyz, rgb = O.cloud_downsample(dm[k], b[k])
        xf = O.bilateral(xyz)
        nrm, dist = O.normals(xf)
        lc, lf, regs = O.segment(xf, nrm)
        out.append(dict(xyz=xf, rgb=rgb, nrm=nrm, dist=dist, lc=lc, lf=lf, regs=regs))
    return out


def cmp_per_pixel(f, ref):
    """Frame f's per-pixel stages and region records against per_sensor_oracle's: cloud, colours, distance map below
    the 9.5 cap it is consumed at, normals, CCL labels, refined labels and every region field, bit for bit."""
    xyz, rgb, nrm, dist = f.cloud()
    lab, labf = f.labels()
    for k in range(8):
        r = ref[k]
        assert same(xyz[k], r["xyz"]), ("cloud", k)
        assert np.array_equal(rgb[k], r["rgb"]), ("rgb", k)
        assert same(np.minimum(dist[k], 9.5), np.minimum(r["dist"], 9.5)), ("dist", k)
        assert same(nrm[k][..., :3], r["nrm"][..., :3]), ("normals", k)
        assert np.array_equal(lab[k], r["lc"]), ("ccl", k)
        assert np.array_equal(labf[k], r["lf"]), ("refined labels", k)
        cmp_regions(f.regions(k), r["regs"], k)


def cmp_regions(regs, oregs, k=None, nan_equal=False):
    """nan_equal: NaN == NaN in the float fields (crafted fields whose regions are lines: the fit of a rank-1
    covariance is NaN in the reference too)."""
    eq = same if nan_equal else np.array_equal
    assert len(regs) == len(oregs), ("regions", k)
    for g, o in zip(regs, oregs):
        assert (g["label"], g["count"], g["start_idx"], g["n_contour"]) == \
            (o["label"], o["count"], o["start_idx"], len(o["contour"])), ("region", k)
        for key in ("centroid", "cov", "model"):
            assert eq(g[key], o[key]), (key, k, g[key], o[key])
        assert eq(g["curvature"], o["curvature"]), (k, g["curvature"], o["curvature"])


def cmp_planes(gp, op):
    assert len(gp) == len(op)
    for g, o in zip(gp, op):
        for key in ("normal", "center", "ppal", "nrgb", "hull"):
            assert np.array_equal(g[key], o[key]), key
        for key in ("d", "area", "elongation", "curvature", "intensity", "id", "sensor", "n_inliers"):
            assert g[key] == o[key], key


# ------------------------------------------------------------------ plane half: ragged sensors and crafted fields
# sensor rows x cols of tests/test_gpu_plane_shapes.py (the organized clouds are rows/2 x cols/2)
PLANE_SHAPES = [(66, 90), (130, 250), (34, 400), (258, 70), (32, 162), (100, 132), (194, 258), (512, 768), (516, 768)]
PLANE_SEEDS = (360 << 16, (360 << 16) + 7)


def plane_pair_rel():
    """The second pose of the synthetic pairs relative to the first: 4 degrees about x and (0, 0.25, 0.15) m."""
    rel = np.eye(4, dtype=np.float32)
    a = np.deg2rad(4.0)
    rel[1:3, 1:3] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    rel[:3, 3] = [0, 0.25, 0.15]
    return rel


def depth_metres(depth_mm):
    """A calibration without intrinsic models leaves depth_m = mm * 0.001f."""
    return depth_mm.astype(np.float32) * np.float32(0.001)


def stripe_sensor(h, w, sw, band=0, phase=0, flip=0):
    """One sensor's organized cloud [h, w, 4] and exact unit normals [h, w, 3] of vertical stripes sw pixels wide (the
    first one sw - phase wide), optionally cut into horizontal bands of `band` rows.  Pixel (v, u) looks along the
    pinhole ray ((u - cx) / f, (v - cy) / f, 1) with f = 525 (2 w / 640) / 2 and centre (w / 2 - 0.5, h / 2 - 0.5);
    stripe k of band b lies on the plane n . p = -2 with n = normalize((+-0.15, 0, -1)), the sign alternating with
    k + b + flip.  Neighbouring stripes' normals differ by 17 degrees (the comparator's threshold is 2.3), so every
    stripe is a label of its own; sw = 0: one plane over the whole sensor."""
    f = 525.0 * (2 * w / 640.0) / 2
    cx, cy = w / 2 - 0.5, h / 2 - 0.5
    v, u = np.mgrid[0:h, 0:w]
    k = (u + phase) // sw if sw else np.zeros_like(u)
    if band:
        k = k + v // band
    sgn = np.where((k + flip) % 2 == 0, 1.0, -1.0)
    ln = np.sqrt(0.15 ** 2 + 1.0)
    n = np.stack([sgn * 0.15 / ln, np.zeros_like(sgn), np.full_like(sgn, -1.0 / ln)], -1)
    ray = np.stack([(u - cx) / f, (v - cy) / f, np.ones((h, w))], -1)
    z = -2.0 / np.einsum("ijk,ijk->ij", ray, n)
    xyz = np.zeros((h, w, 4), np.float32)
    xyz[..., :3] = ray * z[..., None]
    return xyz, n.astype(np.float32)


# the crafted fields of tests/test_gpu_plane_shapes.py: cloud h x w, stripe width, band rows, and the sensors'
# (kind, phase, flip): "s" striped, "p" one plane, "n" all NaN
STRIPE_CASES = {
    # 40 stripes of 84 pixels per striped sensor; sensors 0 and 1 alike, so the 512-pixel span over their seam holds
    # 80 keys (more than the 64 slots of k_gm's table)
    "a": dict(h=21, w=160, sw=4, band=0, sensors=[("s", 0, 0), ("s", 0, 0), ("n", 0, 0), ("p", 0, 0), ("s", 1, 0),
                                                   ("s", 2, 1), ("n", 0, 0), ("s", 3, 0)]),
    # 64 one-pixel stripes of 81 pixels: exactly R360_MAX_MODELS models
    "b": dict(h=81, w=64, sw=1, band=0, sensors=[("s", 0, 0), ("n", 0, 0), ("s", 0, 1), ("p", 0, 0), ("s", 0, 0),
                                                  ("s", 0, 1), ("n", 0, 0), ("s", 0, 0)]),
    # 60 one-pixel stripes of 200 pixels: 23 940 contour points per striped sensor (> TR_LIST)
    "c": dict(h=200, w=60, sw=1, band=0, sensors=[("s", 0, 0), ("p", 0, 0), ("n", 0, 0), ("s", 0, 1), ("s", 0, 0),
                                                   ("n", 0, 0), ("s", 0, 1), ("s", 0, 0)]),
    # 70 models: error bit 4
    "d": dict(h=81, w=70, sw=1, band=0, sensors=[("s", 0, 0), ("n", 0, 0), ("p", 0, 0), ("s", 0, 1), ("s", 0, 0),
                                                  ("s", 0, 1), ("n", 0, 0), ("s", 0, 0)]),
    # 640 labels above 80 points: error bit 2
    "e": dict(h=240, w=320, sw=1, band=81, sensors=[("s", 0, 0), ("n", 0, 0), ("p", 0, 0), ("s", 0, 1), ("s", 0, 0),
                                                     ("s", 0, 1), ("n", 0, 0), ("s", 0, 0)]),
}


def stripe_frame(case, h=None, w=None, sw=None):
    """The 8 sensors' fields of STRIPE_CASES[case] (at another cloud size h x w or stripe width if given): (xyz4 [8, h, w, 4],
    normals [8, h, w, 3], rgb4 [8, h, w, 4] with fixed pseudo-random bytes and a zero fourth byte)."""
    c = STRIPE_CASES[case]
    h, w, sw = h or c["h"], w or c["w"], sw or c["sw"]
    xyz = np.zeros((8, h, w, 4), np.float32)
    nrm = np.zeros((8, h, w, 3), np.float32)
    for s, (kind, phase, flip) in enumerate(c["sensors"]):
        if kind == "n":
            xyz[s, ..., :3] = np.nan
            nrm[s] = np.nan
        else:
            xyz[s], nrm[s] = stripe_sensor(h, w, sw if kind == "s" else 0, c["band"] if kind == "s" else 0,
                                           phase, flip)
    rgb = np.random.default_rng(4242).integers(0, 256, (8, h, w, 4), dtype=np.uint8)
    rgb[..., 3] = 0
    rgb[0, 0, :4, :3] = 0          # black pixels: moments_add_rgb's zero-sum branch
    return xyz, nrm, rgb


def stripe_oracle(xyz, nrm):
    """O.segment per sensor of a crafted frame: [(labels, refined labels, regions)] * 8."""
    from oracle import oracle360 as O
    out = []
    for s in range(8):
        n4 = np.zeros(xyz[s].shape, np.float32)
        n4[..., :3] = nrm[s]
        out.append(O.segment(xyz[s], n4, max_regions=1024))
    return out


def span_keys(labels8, keyed8, px=512):
    """Distinct (sensor, label) keys per span of `px` consecutive pixels of the 8 sensors' label images taken as one
    array (k_gm's workgroups): labels8 [8, h, w]; keyed8[s] = the labels of sensor s that have a key."""
    flat = labels8.reshape(8, -1)
    n = flat.shape[1]
    key = np.full(8 * n, -1, np.int64)
    for s in range(8):
        ok = np.isin(flat[s], np.asarray(sorted(keyed8[s]), np.int64))
        key[s * n:(s + 1) * n] = np.where(ok, s * n + flat[s], -1)
    return [len(set(key[i:i + px].tolist()) - {-1}) for i in range(0, 8 * n, px)]


# ------------------------------------------------------------------ frame front end: undistort, stitch, compaction
# sensor rows x cols of tests/test_gpu_frame_shapes.py -> the pyramid depth the library builds for the sphere they give
# (W = 8 rows, H = int(W / 6); the stitch walks it in 64-row x 16-column tiles, the compaction in 4096-pixel blocks):
#   2x2     2x16    one tile with 2 of its 64 rows live, W / 16 == 1
#   10x14   13x80   odd H, cols % 4 == 2
#   50x70   66x400  a full tile row plus one of 2 rows; 7 compaction blocks, the last partial; W % 64 != 0: never lean
#   56x76   74x448  W % 64 == 0 (a setCompaction(False) frame is lean); a partial second tile row; cols % 4 == 0
#   96x128  128x768 two whole tile rows; lean; exactly 24 compaction blocks; the deepest pyramid
#   100x134 133x800 three tile rows, the last of 5 rows; odd H
FRAME_SHAPES = {(2, 2): 1, (10, 14): 1, (50, 70): 2, (56, 76): 2, (96, 128): 6, (100, 134): 1}
FRAME_LEAN = {(56, 76): True, (96, 128): True, (50, 70): False}
IDENTITY_RTI = np.tile(np.eye(4, dtype=np.float32).reshape(16), 8)   # the poses a calibration holds before it loads any
SRC_BLOCK = 4096                       # pixels per block of the source-point compaction
LIB_PI = 3.14159265359                 # the library's (and the reference's) pi literal


def sphere_size(rows):
    """(H, W) of the sphere stitched from sensors of `rows` rows (Frame360.h:391-392)."""
    W = 8 * rows
    return int(W * 0.5 * 60.0 / 180), W


def pyramid_depth(R, C, cap=6):
    """The number of levels the library builds for an R x C sphere: a level needs 2 rows, 8 columns and a width that
    is a multiple of 4, and an odd level is the last."""
    n = 0
    while n < cap:
        if R < 2 or C < 8 or C % 4:
            break
        n += 1
        if R % 2 or C % 2:
            break
        R, C = R // 2, C // 2
    return n


def frame_images(rows, cols, k=0):
    """8 sensors' BGR in 1..255 and depth in 0..6999 mm with 20 % zeros, seeded from the shape (k: a further set).
    At 6999 mm the stitch's range, depth * sqrt(1 + du^2 + dv^2), stays far below the 65535 of its uint16 cast."""
    rng = np.random.default_rng(100000 * rows + 100 * cols + k)
    b = rng.integers(1, 256, (8, rows, cols, 3), dtype=np.uint8)
    d = rng.integers(0, 7000, (8, rows, cols)).astype(np.uint16)
    d[rng.random((8, rows, cols)) < 0.2] = 0
    return b, d


# synthetic CLAMS models: sensor size, bin size in pixels (after the loaders' downsampleParams(2)), frustums per row
# and column, depth bins and their depth in metres
CLAMS_CASES = {
    # cols % 4 == 2: the scalar kernel
    "50x70": dict(rows=50, cols=70, bin_w=7, bin_h=5, nx=10, ny=10, nb=5, bin_depth=2.0),
    # k_undistort4 with every quad spanning two frustums
    "48x64": dict(rows=48, cols=64, bin_w=2, bin_h=6, nx=32, ny=8, nb=5, bin_depth=2.0),
    # quads that straddle a bin edge at a column that is no multiple of 4 (19, 57); a second table geometry
    "56x76": dict(rows=56, cols=76, bin_w=19, bin_h=7, nx=4, ny=8, nb=3, bin_depth=1.5),
    # bins that do not divide the sensor (nx = ceil(70 / 8), ny = ceil(50 / 6), as the reference sizes its grid): the
    # per-sensor table stride nx * ny is not (rows / bin_h) * nx
    "50x70_ragged_bins": dict(rows=50, cols=70, bin_w=8, bin_h=6, nx=9, ny=9, nb=5, bin_depth=2.0),
}
CLAMS_COUNTS = (0, 49, 50, 51, 1000)   # around the interpolation's `count < 50` test
CLAMS_EDGE_MM = (0, 1, 999, 1000, 1001, 2000, 8000, 8999, 9000, 9999, 10000, 65535)


def clams_tables(name, k):
    """Sensor k's (counts, multipliers) of a case, each float32 [ny, nx, nb]: another seed per sensor."""
    c = CLAMS_CASES[name]
    rng = np.random.default_rng(7000 * c["rows"] + 10 * c["cols"] + 100000 * c["bin_h"] + k)
    shape = (c["ny"], c["nx"], c["nb"])
    counts = rng.choice(np.array(CLAMS_COUNTS, np.float32), shape)
    mult = rng.uniform(0.9, 1.1, shape).astype(np.float32)
    return counts, mult


def write_clams_models(dirpath, name):
    """The case's eight compact model files (the layout tools/compact_clams.py writes) in dirpath; returns their
    paths.  The header holds twice the sensor and bin size: both loaders apply downsampleParams(2)."""
    import os
    import struct
    c = CLAMS_CASES[name]
    paths = []
    for k in range(8):
        counts, mult = clams_tables(name, k)
        p = os.path.join(str(dirpath), f"distortion_model{k + 1}.r360")
        with open(p, "wb") as f:
            f.write(b"R360CLAMS1\n")
            f.write(struct.pack("<iiiiiiid", 2 * c["cols"], 2 * c["rows"], 2 * c["bin_w"], 2 * c["bin_h"], c["nx"],
                                c["ny"], c["nb"], c["bin_depth"]))
            f.write(counts.tobytes())
            f.write(mult.tobytes())
        paths.append(p)
    return paths


def clams_depth(name):
    """8 sensors' depth in 0..11999 mm with 10 % zeros; the first pixels of sensor 0 are CLAMS_EDGE_MM."""
    c = CLAMS_CASES[name]
    rng = np.random.default_rng(31 * c["rows"] + c["cols"] + 1000 * c["bin_h"])
    d = rng.integers(0, 12000, (8, c["rows"], c["cols"])).astype(np.uint16)
    d[rng.random(d.shape) < 0.1] = 0
    d[0].reshape(-1)[:len(CLAMS_EDGE_MM)] = CLAMS_EDGE_MM
    return d


def clams_branches(name, z, counts):
    """The branch each pixel of one sensor takes in the undistortion (discrete_depth_distortion_model.cpp:175-186,
    48-68), restated in numpy: z float32 [rows, cols] in metres, counts [ny, nx, nb].  Boolean masks; `zero`, `idx0_neg`,
    `idx1_past`, `low_count` and `interpolated` partition the image in the order the code tests them, `past_last_bin`
    (a depth whose bin index is clamped) lies inside `idx1_past`."""
    c = CLAMS_CASES[name]
    nb, bd = c["nb"], c["bin_depth"]
    v, u = np.mgrid[0:c["rows"], 0:c["cols"]]
    cnt = counts[v // c["bin_h"], u // c["bin_w"]]                       # [rows, cols, nb]
    raw = np.floor(z.astype(np.float64) / bd).astype(np.int64)
    idx = np.minimum(raw, nb - 1)
    start = (bd * idx).astype(np.float32)
    idx1 = np.where((z - start).astype(np.float64) < bd / 2, idx, idx + 1)
    idx0 = idx1 - 1
    take = lambda i: np.take_along_axis(cnt, np.clip(i, 0, nb - 1)[..., None], axis=2)[..., 0]
    zero = z == 0
    idx0_neg = ~zero & (idx0 < 0)
    idx1_past = ~zero & ~idx0_neg & (idx1 >= nb)
    rest = ~zero & ~idx0_neg & ~idx1_past
    low = rest & ((take(idx0) < 50) | (take(idx1) < 50))
    return dict(zero=zero, idx0_neg=idx0_neg, idx1_past=idx1_past, low_count=low, interpolated=rest & ~low,
                past_last_bin=~zero & (raw > nb - 1))


def src_points_model(lv):
    """The compacted source points of a pyramid level (the oracle's {gray, depth}) stated in float64: for the pixels
    with float32(0.3) < d < float32(6.0), in raster order, (gray float32 [n], points float64 [n, 3], d float32 [n]) with
    the point (d sin phi_r, -d cos phi_r sin theta_c, -d cos phi_r cos theta_c).  phi_r and theta_c are the float32
    angles the library's tables are built from; their sines and cosines are taken in float64."""
    d, g = np.asarray(lv["depth"], np.float32), np.asarray(lv["gray"], np.float32)
    R, C = d.shape
    ares = np.float32(2 * LIB_PI / C)
    phi = ((np.float32(0.5 * R - 0.5) - np.arange(R, dtype=np.float32)) * ares).astype(np.float32)
    theta = (np.arange(C, dtype=np.float32) * ares).astype(np.float32)
    valid = (d > np.float32(0.3)) & (d < np.float32(6.0))
    r, c = np.nonzero(valid)
    dv = d[valid]
    d64, ph, th = dv.astype(np.float64), phi[r].astype(np.float64), theta[c].astype(np.float64)
    pts = np.stack([d64 * np.sin(ph), -d64 * np.cos(ph) * np.sin(th), -d64 * np.cos(ph) * np.cos(th)], axis=1)
    return g[valid], pts, dv


SRC_GATE_MM = (0, 299, 300, 301, 5999, 6000, 6001)   # around the strict 0.3 < d < 6.0 gate
CRAFTED_SPHERES = [(66, 400), (128, 768)]
CRAFTED_KINDS = ("blocks", "zeros", "gate")


def crafted_sphere(rows, cols, kind):
    """A sphere as images whose ranges are made for the compaction: "blocks": raster pixels 4096..8191 (block 1) all
    invalid (0, 299 and 6001 mm by turns), 8192..12287 (block 2) all valid, noise elsewhere; "zeros": every range 0;
    "gate": every range one of SRC_GATE_MM."""
    rng = np.random.default_rng(17 * rows + cols + len(kind))
    bgr = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    if kind == "zeros":
        dep = np.zeros((rows, cols), np.uint16)
    elif kind == "gate":
        dep = rng.choice(np.array(SRC_GATE_MM, np.uint16), (rows, cols))
    else:
        dep = rng.integers(0, 7000, (rows, cols)).astype(np.uint16)
        dep[rng.random((rows, cols)) < 0.2] = 0
        flat = dep.reshape(-1)
        flat[SRC_BLOCK:2 * SRC_BLOCK] = np.resize(np.array([0, 299, 6001], np.uint16), SRC_BLOCK)
        flat[2 * SRC_BLOCK:3 * SRC_BLOCK] = rng.integers(400, 5900, SRC_BLOCK).astype(np.uint16)
    return bgr, dep


# ------------------------------------------------------------------ per-sensor dense paths: pinhole and rig-frame passes
# sensor rows x cols of tests/test_gpu_sensor_shapes.py -> the levels of the per-sensor pyramid the library builds
# (halve while both sizes are even and at least 8, at most SENSOR_MAX_PYR levels); the last level:
#   2x2     2x2    four pixels, every gradient zero, H = 0
#   10x14   5x7    both levels below one workgroup, level 1 below one wave: tail pixels only
#   50x70   25x35  odd in both directions; 3500 px = 4 workgroups, 3.4 strides
#   56x76   14x19  odd columns only; 28x38: 2 workgroups, 2.08 strides; 14x19 = 266 px: 10 threads pair, the rest tail
#   96x128  6x8    exactly 4 strides at levels 0 and 1 (pairs only); the last level below one wave; 40 rig-frame jobs
#   100x134 50x67  odd columns at level 1; 14 workgroups, 3.74 strides
#   120x160 15x20  odd rows only at the last level; 19 workgroups
SENSOR_SHAPES = {(2, 2): 1, (10, 14): 2, (50, 70): 2, (56, 76): 3, (96, 128): 5, (100, 134): 2, (120, 160): 4}
SENSOR_MAX_PYR = 6                     # R360_MAX_PYR
PASS_TPB, PASS_PPT, PASS_MAX_BLOCKS = 256, 4, 256   # threads per workgroup, pixels per thread, workgroups per job
SENSOR_CAPTURES = {"dec": 4, "crop": 3}             # the decimated / cropped sample captures -> their level count


def sensor_levels(rows, cols, cap=SENSOR_MAX_PYR):
    """[(rows, cols)] of the per-sensor pyramid of a rows x cols sensor."""
    out = []
    while len(out) < cap:
        out.append((rows, cols))
        if rows % 2 or cols % 2 or rows < 8 or cols < 8:
            break
        rows, cols = rows // 2, cols // 2
    return out


def sensor_images(rows, cols, which):
    """`noise` images of 8 sensors: BGR uniform, depth uniform in 0..6999 mm with 20 % zeros.  which: "target", "source" or
    "other" (a third set), each from a seed of its own derived from the shape."""
    rng = np.random.default_rng(1000003 * rows + 1009 * cols + ("target", "source", "other").index(which))
    b = rng.integers(0, 256, (8, rows, cols, 3), dtype=np.uint8)
    d = rng.integers(0, 7000, (8, rows, cols)).astype(np.uint16)
    d[rng.random((8, rows, cols)) < 0.2] = 0
    return b, d


def sensor_captures(kind, samples_dir):
    """((target BGR, depth), (source BGR, depth)) of the two QVGA sample captures, "dec": decimated [:, ::2, ::2] to
    8 x 120 x 160; "crop": cropped [:, 92:148, 122:198] to 8 x 56 x 76."""
    import os
    from oracle import oracle360 as O
    out = []
    for name in ("sphere_images_1.bin", "sphere_images_10.bin"):
        b, d = O.load_bin(os.path.join(samples_dir, name))
        if kind == "dec":
            b, d = b[:, ::2, ::2], d[:, ::2, ::2]
        else:
            b, d = b[:, 92:148, 122:198], d[:, 92:148, 122:198]
        out.append((np.ascontiguousarray(b), np.ascontiguousarray(d)))
    return tuple(out)


# (translation, rotation) twists: the two of test_gpu_pinhole._poses() and a larger motion, 0.45 rad about y (a shift of
# 525 tan(0.45) = 254 of the 640 columns' worth of focal length: about 0.4 of the width leaves the image).  No point goes
# behind the camera: a pixel's ray is at most atan(hypot(320, 240) / 525) = 37.3 degrees off the axis (less on the
# narrower shapes), the rotation is 26.4 degrees, so Z >= 0.3 cos(63.7 deg) - 0.05 > 0.08 m
# (tests/test_oracle_sensor_shapes.py checks it on every pixel).
SENSOR_TWISTS = ([0.01, -0.02, 0.015, 0.01, -0.005, 0.008], [-0.05, 0.03, -0.04, -0.02, 0.03, -0.01],
                 [0.03, -0.02, 0.04, 0.08, 0.45, -0.06])
SENSOR_LARGE_POSE = 3                  # index into sensor_poses()


def sensor_poses():
    """The identity, test_gpu_pinhole._poses()'s two twists and the larger motion (true SE(3) exponentials)."""
    from oracle import oracle360 as O
    return [np.eye(4, dtype=np.float32)] + [O.exp_se3(t, pseudo=False).astype(np.float32) for t in SENSOR_TWISTS]


def pass_blocks(npx):
    """Workgroups per job of a pinhole or rig-frame pass over npx pixels."""
    return max(1, min(PASS_MAX_BLOCKS, -(-npx // (PASS_TPB * PASS_PPT))))


def pin_thread_classes(npx):
    """k_pin_pass's loop restated per thread: thread t of the nb * 256 of a job starts at pixel t, takes pixels i and
    i + stride while i + stride < npx (i += 2 stride), then pixel i alone if i < npx.  Returns the thread counts
    dict(idle, tail_only, pair_only, pair_and_tail) and the pixels covered (which must be npx)."""
    stride = pass_blocks(npx) * PASS_TPB
    out = dict(idle=0, tail_only=0, pair_only=0, pair_and_tail=0)
    covered = 0
    for t in range(stride):
        i, pairs = t, 0
        while i + stride < npx:
            pairs += 1
            i += 2 * stride
        tail = i < npx
        covered += 2 * pairs + tail
        out["pair_and_tail" if pairs and tail else "pair_only" if pairs else "tail_only" if tail else "idle"] += 1
    return out, covered


def _pose_diff(A, B):
    from oracle import oracle360 as O
    return O.rot_angle(A[:3, :3], B[:3, :3]), float(np.linalg.norm(A[:3, 3] - B[:3, 3]))


_CENSUS = {}


def sensor_align_census(kind, method, samples_dir):
    """The oracle's alignFrames of the 8 sensors of a capture pair from the identity, and each solve's stability: from
    each of the 12 starts exp(+-1e-7 e_i), i = 1..6, the oracle returns the same rc and a pose within 1e-4 rad and
    1e-3 m of its unperturbed answer (test_gpu_pinhole._oracle_stable's rule, twelve nudges instead of one).  Per
    sensor dict(ref=(rc, pose, H, g, stats), stable, drift=(rad, m) the largest over the nudges, derr = the largest
    change of the final error under them).  Computed once per process and left unchanged."""
    from oracle import oracle360 as O
    key = (kind, method)
    if key in _CENSUS:
        return _CENSUS[key]
    (bt, dt), (bs, ds) = sensor_captures(kind, samples_dir)
    p = O.IcpParams.default(n_pyr=SENSOR_CAPTURES[kind])
    eye = np.eye(4, dtype=np.float32)
    out = []
    for k in range(8):
        ref = O.align_pinhole(bt[k], dt[k], bs[k], ds[k], init=eye, method=method, params=p)
        stable, dr_max, dt_max, derr = True, 0.0, 0.0, 0.0
        for i in range(6):
            for s in (1e-7, -1e-7):
                tw = np.zeros(6)
                tw[i] = s
                rc, Pp, _, _, stp = O.align_pinhole(bt[k], dt[k], bs[k], ds[k],
                                                    init=O.exp_se3(tw, pseudo=False).astype(np.float32), method=method,
                                                    params=p)
                dr, dtr = _pose_diff(Pp, ref[1])
                stable = stable and rc == ref[0] and dr <= 1e-4 and dtr <= 1e-3
                dr_max, dt_max = max(dr_max, dr), max(dt_max, dtr)
                derr = max(derr, abs(stp.error - ref[4].error))
        out.append(dict(ref=ref, stable=stable, drift=(dr_max, dt_max), derr=derr))
    _CENSUS[key] = out
    return out
