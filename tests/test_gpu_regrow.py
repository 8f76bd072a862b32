"""Buffers that grow on demand give the results of buffers that never grew (MI355X).

Contexts and handles regrow their device and pinned memory when a call needs more (the pose graph's and the rig
calibration's handles through DevBuf / PinnedBuf, rgbd360_amd/csrc/host/devmem.h).  Each case drives one context, or one handle, small -> large -> small across
the growth rules of its buffers (the 1024-item floors of the voxel grid and GICP, the map's half-as-much-again step,
the per-graph and per-row sizes of the pose graph and the rig calibration, one chunk more than R360_TOPO_CHUNK, the
per-pixel occlusion buffers and deferred queues, the batch set) and compares every result bit for bit (_cases.same)
with the same call on a fresh context or handle.  One case creates and destroys contexts that ran an occlusion
alignment.  The last two do the same with the handles whose buffers are sized once: calibrations and frames of two
sensor sizes, fully built, created and destroyed in turn and with overlapping lifetimes.  Nothing here makes an
allocation fail: those paths are tests/test_devmem_host.py's."""
import contextlib

import numpy as np
import pytest

import rgbd360_amd as R

import _gicp_cases as GC
import _pgo_cases as PC
import _rigcal_cases as RC
import _topo_cases as TC
from _cases import PLANE_SEEDS, PLANE_SHAPES, noise_sphere, same, sensor_levels
from test_gpu_voxel import _check_against_model

pytestmark = pytest.mark.gpu

TOPO_CHUNK = 32   # R360_TOPO_CHUNK


@contextlib.contextmanager
def context():
    c = R.Context(0)
    try:
        yield c
    finally:
        c.close()


def _same_all(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert same(x, y), (what, k)


# ------------------------------------------------------------------ Generalized-ICP
def _gicp(ctx, n):
    p = R.GicpParams.default()
    p.max_corr_dist = 2.0          # 200 points on 108 m^2 of walls lie 0.7 m apart
    s, t = GC.pair(n, n)
    ctx.gicp_set_source(s, p)
    ctx.gicp_set_target(t, p)
    pose, st, rc = ctx.gicp_align(np.eye(4), p)
    assert rc == 0 and st.n_corr > 0
    return [pose, np.frombuffer(bytes(st), np.uint8), rc]


def test_gicp_clouds_across_the_floor():
    """200, 1500, 200 points: source, target and the pass buffers start at the 1024-item floor and grow past it."""
    with context() as used:
        got = [_gicp(used, n) for n in (200, 1500, 200)]
    for n, g in zip((200, 1500, 200), got):
        with context() as fresh:
            _same_all(g, _gicp(fresh, n), f"gicp {n}")


# ------------------------------------------------------------------ voxel filter and the context's map
def _cloud(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-3, 3, (n, 3)).astype(np.float32), rng.integers(0, 1 << 24, n).astype(np.uint32)


def test_voxel_filter_across_the_floor():
    sizes = (500, 3000, 500)
    with context() as used:
        got = [used.filter_voxel(*_cloud(n, n)) for n in sizes]
    for n, g in zip(sizes, got):
        with context() as fresh:
            w = fresh.filter_voxel(*_cloud(n, n))
        assert g[2] and w[2]
        _same_all(g[:2], w[:2], f"voxel filter {n}")
        _check_against_model(*_cloud(n, n), 0.05, g[0], g[1])


def test_map_takes_a_geometric_step():
    """Three clouds of 600 points, nearly every one a voxel of its own: the map needs 600, about 1200 and about 1800
    points, so its buffers start at 1024, then grow by half (1536), then again."""
    clouds = [_cloud(600, 10 + k) for k in range(3)]
    out = []
    for _ in range(2):
        with context() as ctx:
            steps = []
            for x, c in clouds:
                assert ctx.map_add_cloud(x, c, 0.05)
                steps.append(ctx.map_download())
            out.append(steps)
    mx, mc = np.zeros((0, 3), np.float32), np.zeros(0, np.uint32)
    for k, ((x, c), a, b) in enumerate(zip(clouds, *out)):
        _same_all(a, b, f"map after cloud {k}")
        _check_against_model(np.vstack([mx, x]), np.concatenate([mc, c]), 0.05, a[0], a[1])
        mx, mc = a
    assert len(mx) > 1536


# ------------------------------------------------------------------ pose graph
def _graph(ctx, poses, edges):
    pg = R.PoseGraph(ctx)
    for T in poses:
        pg.addVertex(T)
    for (i, j, Z, Om) in edges:
        pg.addEdge(i, j, Z, Om)
    return pg


def _optimised(pg):
    st = pg.optimizeGraph()
    assert st.iterations > 0
    return [pg.getPoses(), np.frombuffer(bytes(st), np.uint8)]


def test_pose_graph_grows_with_its_graph():
    """4 vertices (a chain and one loop edge, so there is something to optimise), then 40 on the same handle."""
    full, truth = PC.build_sized(40, 4, [(0, 20), (0, 39), (10, 30)])
    rng = np.random.default_rng(4)
    small = [e for e in full.edges if max(e[0], e[1]) <= 3] + [(0, 3, PC.measure(rng, truth[0], truth[3], 0.002, 0.0006),
                                                                 PC.info(rng))]
    rest = [e for e in full.edges if max(e[0], e[1]) > 3]
    with context() as ctx:
        pg = _graph(ctx, full.poses[:4], small)
        first = _optimised(pg)
        for T in full.poses[4:]:
            pg.addVertex(T)
        for (i, j, Z, Om) in rest:
            pg.addEdge(i, j, Z, Om)
        start = pg.getPoses()
        grown = _optimised(pg)
        fresh = _graph(ctx, list(start), small + rest)
        _same_all(grown, _optimised(fresh), "40 vertices: grown handle against a fresh one")
        again = _graph(ctx, full.poses[:4], small)
        _same_all(first, _optimised(again), "4 vertices after 40 on the same context")
        for g in (pg, fresh, again):
            g.close()


# ------------------------------------------------------------------ rig calibration
def _solved(cal):
    a = cal.CalibrateRotation(True)
    b = cal.CalibrateTranslation(True)
    H, g, sc = cal.eval(0, True)
    return [np.frombuffer(bytes(a), np.uint8), np.frombuffer(bytes(b), np.uint8), cal.estimate(), H, g, sc]


def test_rig_calibration_grows_with_its_rows():
    """The seven adjacent pairs at 3 rows (7 workgroups), then a pair of 300 rows beside them (9 workgroups: more rows,
    a longer workgroup table, more records)."""
    rig = RC.perturbed_rig(5)
    few = RC.make_rows(rig, RC.base_counts(), 11, noise=1e-3)
    more = RC.make_rows(rig, {(0, 2): 300}, 12, noise=1e-3)
    specs = R.rigcal_specs()
    with context() as ctx:
        cal = R.RigCalibration(ctx)
        cal.setPairs(few)
        first = _solved(cal)
        cal.setPair(0, 2, more[(0, 2)])
        cal.setInit(specs)             # the second solve starts where a fresh handle's does
        grown = _solved(cal)
        fresh = R.RigCalibration(ctx)
        fresh.setPairs({**few, **more})
        _same_all(grown, _solved(fresh), "all rows: grown handle against a fresh one")
        again = R.RigCalibration(ctx)
        again.setPairs(few)
        _same_all(first, _solved(again), "the few rows after the many on the same context")
        for h in (cal, fresh, again):
            h.close()


# ------------------------------------------------------------------ topological partition
def test_topo_one_chunk_more():
    six = TC.rooms_graph(6, 2, 3)
    batch = [TC.rooms_graph(5 + k % 7, 2, 100 + k) for k in range(TOPO_CHUNK + 1)]
    with context() as used:
        got = [R.topo_partition(used, six, return_cuts=True), R.topo_partition_batch(used, batch),
               R.topo_partition(used, six, return_cuts=True)]
    with context() as fresh:
        _same_all(got[0], R.topo_partition(fresh, six, return_cuts=True), "6 nodes first")
    with context() as fresh:
        _same_all(got[1], R.topo_partition_batch(fresh, batch), "33 graphs")
    with context() as fresh:
        _same_all(got[2], R.topo_partition(fresh, six, return_cuts=True), "6 nodes after 33 graphs")


# ------------------------------------------------------------------ dense alignments
GEOMS = {"64x384": (64, 384, 6), "80x576": (80, 576, 5)}   # rows, columns, levels (tests/test_gpu_icp_shapes.py)


def _pair(ctx, name, seed=0):
    rows, cols, n = GEOMS[name]
    cal = R.Calib360.for_sphere(ctx, rows, cols)
    frames = []
    for k in range(2):
        f = R.Frame360(cal)
        f.set_sphere(*noise_sphere(rows, cols, 1000 * rows + cols + 2 * seed + k))
        frames.append(f)
    return cal, frames


def _params(name):
    p = R.IcpParams.default()
    p.n_pyr = min(p.n_pyr, GEOMS[name][2])
    return p


def _align(ctx, name, occ):
    cal, (t, s) = _pair(ctx, name)
    reg = R.RegisterPhotoICP(ctx)
    reg.params = _params(name)
    reg.setTargetFrame(t)
    reg.setSourceFrame(s)
    rc = reg.alignFrames360(np.eye(4), R.PHOTO_DEPTH, occ)
    out = [rc, reg.getOptimalPose().copy(), reg.getHessian().copy(), reg.getGradient().copy(),
           list(reg.stats.iters), list(reg.stats.evals)]
    for f in (t, s):
        f.close()
    cal.close()
    return out


@pytest.mark.parametrize("occ", [1, 2])
def test_occlusion_alignment_across_sizes(occ):
    """64x384, 80x576, 64x384: the seven per-pixel occlusion buffers and the deferred-pixel queue grow at the second."""
    names = ("64x384", "80x576", "64x384")
    with context() as used:
        got = [_align(used, name, occ) for name in names]
    for name, g in zip(names, got):
        with context() as fresh:
            _same_all(g, _align(fresh, name, occ), f"occlusion {occ} at {name}")


def _batch(ctx, frames, n):
    pairs = [(frames[2 * j], frames[2 * j + 1]) for j in range(n)]
    poses, H, g, st, ill = R.align360_batch(ctx, pairs, None, R.PHOTO_DEPTH, _params("64x384"))
    return [poses, H, g, np.frombuffer(b"".join(bytes(s) for s in st), np.uint8), ill]


def test_batched_alignment_across_batch_sizes():
    """One pair, three pairs, one pair at 64x384: the batch set (states, records, tickets, queues) grows at the second."""
    @contextlib.contextmanager
    def three_pairs(ctx):
        made = [_pair(ctx, "64x384", seed) for seed in range(3)]
        try:
            yield [f for _, pair in made for f in pair]
        finally:
            for cal, pair in made:
                for f in pair:
                    f.close()
                cal.close()

    with context() as used, three_pairs(used) as frames:
        got = [_batch(used, frames, n) for n in (1, 3, 1)]
    for n, g in zip((1, 3, 1), got):
        with context() as fresh, three_pairs(fresh) as frames:
            _same_all(g, _batch(fresh, frames, n), f"batch of {n}")


def test_context_churn():
    """Create, align with occlusion, destroy, eight times: the eighth result is the first."""
    runs = []
    for _ in range(8):
        with context() as ctx:
            runs.append(_align(ctx, "64x384", 1))
    _same_all(runs[0], runs[7], "context churn")


# ------------------------------------------------------------------ calibrations and frames
FRAME_SHAPES = [(66, 90), (32, 162)]
assert set(FRAME_SHAPES) <= set(PLANE_SHAPES)
FULL_BUILD = (R.BUILD_UNDISTORT | R.BUILD_SPHERE | R.BUILD_PYRAMID | R.BUILD_SENSOR_PYRAMID | R.BUILD_CLOUD |
              R.BUILD_PLANES)
_IMAGES = {}


def _images(cal, shape, seed):
    """The synthetic room's 8 sensor images at `shape`, rendered once (on the host) and left unchanged."""
    if (shape, seed) not in _IMAGES:
        _IMAGES[shape, seed] = cal.synth_frame(seed, R.synth_path_pose(seed, 0))
    return _IMAGES[shape, seed]


def _sphere_levels(rows, cols):
    n = 0
    while n < 6 and rows >= 2 and cols >= 8 and cols % 4 == 0:
        n += 1
        if rows % 2 or cols % 2:
            break
        rows, cols = rows // 2, cols // 2
    return n


def _built_frame(ctx, shape, seed=PLANE_SEEDS[0]):
    """Calibration and frame created, images uploaded, everything built: sphere, pyramid, sensor pyramid, planes."""
    cal = R.Calib360(ctx, *shape)
    cal.loadExtrinsicCalibration(R.EXTRINSICS_DIR)
    f = R.Frame360(cal)
    f.upload(*_images(cal, shape, seed))
    f.build(FULL_BUILD)
    return cal, f


def _read_back(f, shape):
    """The sphere's level images, the sensors' (sensors 0 and 7), the sensors' clouds, the labels, the regions and the
    planes, as arrays."""
    n = _sphere_levels(f.sph_rows, f.sph_cols)
    assert n >= 2
    out = list(f.sphere())
    for l in range(n):
        out += list(f.level(l).values())
    for l in range(len(sensor_levels(*shape))):
        for k in (0, 7):
            out += list(f.sensor_level(k, l).values())
    out += list(f.cloud()) + list(f.labels())
    # (at these sizes a sensor's cloud has few labels above the 80-point bar, and may have no region at all)
    for d in [r for k in range(8) for r in f.regions(k)] + f.planes():
        out += [np.asarray(d[key]) for key in sorted(d)]
    return out


def _drop(cal, f):
    f.close()
    cal.close()


def test_frame_churn():
    """Eight times at each of two sensor sizes: calibration and frame created, uploaded, fully built, read back,
    destroyed.  The eighth read-back is the first, bit for bit."""
    with context() as ctx:
        for shape in FRAME_SHAPES:
            runs = []
            for _ in range(8):
                cal, f = _built_frame(ctx, shape)
                runs.append(_read_back(f, shape))
                _drop(cal, f)
            _same_all(runs[0], runs[7], f"frame churn at {shape}")


def test_frames_with_overlapping_lifetimes():
    """A and B built, A destroyed, C created and built at the other size where A's memory was: B reads back as before,
    and C as on a fresh context."""
    small, wide = FRAME_SHAPES
    with context() as ctx:
        cal_a, a = _built_frame(ctx, small)
        cal_b, b = _built_frame(ctx, small, PLANE_SEEDS[1])
        before = _read_back(b, small)
        _drop(cal_a, a)
        cal_c, c = _built_frame(ctx, wide)
        got = _read_back(c, wide)
        _same_all(before, _read_back(b, small), "B after A went and C came")
        _drop(cal_b, b)
        _drop(cal_c, c)
    with context() as fresh:
        cal_c, c = _built_frame(fresh, wide)
        _same_all(got, _read_back(c, wide), "C against a fresh context")
        _drop(cal_c, c)
