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
