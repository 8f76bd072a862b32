"""Every form of the fused ICP pass (k_icp_pass: PF 6, 5, 8, 9 for the plain pass, PF 3 / PF 0 for the occlusion
variants) on small ragged spheres, on the lone grid and on the batched one, against the CPU oracle.

The form and the grid of a pass come from the level's shape (pass_grid, icp_kernels.hip), and the kernels have
shape-dependent code that the samples' and the synthetic pairs' levels (120 * 2^k columns, 20 * 2^k rows) never vary:
PF 9's wrap of a wave over a row end, row_of's float division, partial last waves that read past the image through
buffer bounds, the clamped tail chunk of the software pipeline with an odd / even / single chunk count, the deferred
queues' capacity, the ticket-group reduction with fewer workgroups than groups or a ragged last round, and the
NaN asin_out of tall spheres (H > 0.175 W), where the fast projection defers every lane past 32 degrees.

Spheres (rows x cols, levels the library builds) and what each is here for:

  20x72     2  a wave always spans two rows; 1440 px = 22.5 waves; level 1 is 10x36
  16x64     4  H = W / 4 (tall); one wave per row
  32x64     4  H = W / 2 (tall)
  40x256    4  levels 1 and 2 (128 and 64 columns) run PF 8 with two waves and one wave per row; level 3 is 5x32
  52x416    3  6.5 waves per row; level 2 is 13x104 (odd row count)
  64x384    6  columns 384 / 192 / 96 / 48 / 24 / 12
  80x576    5  columns 576 / 288 / 144 / 72 / 36
  130x1040  2  135200 px > 2 x CUs x 256: the lone grid is capped and strides with 1 and 2 chunks; level 1 is 65x520

Each is built with every level's source points compacted (the default: a lone pass runs PF 5) and with
setCompaction(False) (the sequence runner's ring frames: the image is streamed wherever a form exists for it).  The
forms and grids the launcher picks are asserted (r360_icp_pass_grid), so a change of the selection cannot silently
take a form out of this file.

Bars: the suite's own (icp_check of _cases.py: counts exact, H 1e-5 of max |H|, g 1e-5 of sqrt(H_kk e2), e2 1e-6; for
the occlusion variants those of test_gpu_occlusion.test_occlusion_pass_parity).  Batched results are bit-identical in
any batch and slot; repeats on one context are bit-identical; whole alignments meet the north-star bar against the
oracle's alignFrames360."""
import functools

import numpy as np
import pytest

import rgbd360_amd as R
from oracle import oracle360 as O
from _cases import ROOM_MOTION, ROOM_SOURCE, ROOM_TARGET, icp_check, noise_sphere, room_pair, room_sphere

pytestmark = pytest.mark.gpu

ROT_TOL, TRANS_TOL = 1e-4, 1e-3
TPB = 256                    # threads per workgroup of k_icp_pass
TICKET_GROUPS = 16           # R360_TICKET_GROUPS

# sphere rows, columns, levels the library builds
GEOMS = {"20x72": (20, 72, 2), "16x64": (16, 64, 4), "32x64": (32, 64, 4), "40x256": (40, 256, 4),
         "52x416": (52, 416, 3), "64x384": (64, 384, 6), "80x576": (80, 576, 5), "130x1040": (130, 1040, 2)}
# plain pass forms of a lone pass over frames built with setCompaction(False), level 0 first
STREAMED = {"64x384": [6, 8, 9, 5, 5, 5], "80x576": [6, 9, 9, 9, 5], "52x416": [5, 9, 9], "20x72": [5, 5],
            "16x64": [6, 5, 5, 5], "32x64": [6, 5, 5, 5], "130x1040": [5, 9], "40x256": [6, 8, 8, 5]}
# batched launches: the same, but a level 0 the packed image cannot serve (cols % 64 != 0) is streamed as PF 9
BATCHED = {k: ([9] + v[1:] if k in ("52x416", "20x72", "130x1040") else list(v)) for k, v in STREAMED.items()}
KINDS = ("room", "noise")
# (geometry, pair, level) of the pass parity test.  "solid" is the room without holes, at 130x1040 only: every pixel is
# a valid source point, so the lone PF 5 pass over the compacted points (135200 > 512 x 256) strides too, with 1 and 2
# chunks
PARITY = [(name, kind, l) for name in GEOMS for kind in KINDS + (("solid",) if name == "130x1040" else ())
          for l in range(GEOMS[name][2])]
POSES = [np.eye(4, dtype=np.float32), O.exp_se3([0.02, -0.03, 0.05, 0.01, -0.015, 0.02])]


@functools.lru_cache(maxsize=None)
def images(name, kind):
    """((target BGR, range), (source BGR, range)) of a geometry."""
    rows, cols, _ = GEOMS[name]
    if kind == "room":
        return room_pair(rows, cols)
    if kind == "solid":
        return tuple(room_sphere(rows, cols, eye, seed, holes=0.0) for eye, seed in (ROOM_TARGET, ROOM_SOURCE))
    return noise_sphere(rows, cols, 1000 * rows + cols), noise_sphere(rows, cols, 1000 * rows + cols + 1)


@functools.lru_cache(maxsize=None)
def pyramids(name, kind):
    (tb, td), (sb, sd) = images(name, kind)
    n = GEOMS[name][2]
    return O.sphere_pyramid(tb, td, n), O.sphere_pyramid(sb, sd, n)


@functools.lru_cache(maxsize=None)
def oracle_pass(name, kind, level, method, pose, occ):
    """The oracle's pass at POSES[pose]: (H, g, e2 or the Occ error value, n_valid, n_visible)."""
    pt, ps = pyramids(name, kind)
    lt, ls, P = pt[level], ps[level], POSES[pose]
    if occ == 0:
        _, e2, nv = O.error_sphere(ls, lt, P, method)
        H, g, nvis = O.hessgrad_sphere(ls, lt, P, method)
        return H, g, e2, nv, nvis
    e, nv = O.error_sphere_occ(ls, lt, P, method, occ)
    H, g, nvis = O.hessgrad_sphere_occ(ls, lt, P, method, occ)
    return H, g, e, nv, nvis


@pytest.fixture(scope="module")
def ctx():
    return R.Context(0)


@pytest.fixture(scope="module")
def bank(ctx):
    """(target, source) frames of a geometry, pair kind and compaction setting, built on first use and kept."""
    calibs, frames = {}, {}

    def get(name, kind, compact):
        key = (name, kind, compact)
        if key not in frames:
            rows, cols, n = GEOMS[name]
            if name not in calibs:
                calibs[name] = R.Calib360.for_sphere(ctx, rows, cols)
            pair = []
            for bgr, dep in images(name, kind):
                f = R.Frame360(calibs[name])
                if not compact:
                    f.setCompaction(False)
                f.set_sphere(bgr, dep)
                pair.append(f)
            with pytest.raises(RuntimeError):   # the library builds the levels this file lists, no more
                pair[0].level(n)
            frames[key] = tuple(pair)
        return frames[key]

    yield get
    for pair in frames.values():
        for f in pair:
            f.close()


def _prm(name):
    """Default parameters with n_pyr at the geometry's pyramid depth (the library refuses a deeper one)."""
    p = R.IcpParams.default()
    p.n_pyr = min(p.n_pyr, GEOMS[name][2])
    return p


def _reg(ctx, name, trg, src):
    reg = R.RegisterPhotoICP(ctx)
    reg.params = _prm(name)
    reg.setTargetFrame(trg)
    reg.setSourceFrame(src)
    return reg


def _grids(ctx, bank, name):
    """{(mode, level): (pf, nb)} for mode in compacted / streamed / batched / occ1 / occ2."""
    n = GEOMS[name][2]
    out = {}
    for compact, mode in ((True, "compacted"), (False, "streamed")):
        reg = _reg(ctx, name, *bank(name, "room", compact))
        for l in range(n):
            out[(mode, l)] = reg.pass_grid(l, 0, False)
            if not compact:
                out[("batched", l)] = reg.pass_grid(l, 0, True)
            else:
                assert reg.pass_grid(l, 0, True)[0] == BATCHED[name][l]   # the batched form ignores compaction
                for occ in (1, 2):
                    out[(f"occ{occ}", l)] = reg.pass_grid(l, occ, False)
    return out


def _want_nb(npx, batched):
    """pass_grid's workgroups per job below its cap: one pixel per thread lone, eight batched."""
    per = TPB * (8 if batched else 1)
    return (npx + per - 1) // per


@pytest.mark.parametrize("name", list(GEOMS))
def test_pass_form_table(ctx, bank, name):
    """The forms and grids the launcher picks for every level of the geometry."""
    rows, cols, n = GEOMS[name]
    G = _grids(ctx, bank, name)
    assert [G[("compacted", l)][0] for l in range(n)] == [5] * n
    assert [G[("streamed", l)][0] for l in range(n)] == STREAMED[name]
    assert [G[("batched", l)][0] for l in range(n)] == BATCHED[name]
    for l in range(n):
        c = cols >> l
        npx = (rows >> l) * c
        for occ in (1, 2):
            assert G[(f"occ{occ}", l)][0] == (3 if c % 64 == 0 else 0), (l, occ)
        # the grid depends on the level's size only (never on the form or the frames), a fixed number per level
        lone = {G[(m, l)][1] for m in ("compacted", "streamed", "occ1", "occ2")}
        assert len(lone) == 1, (l, lone)
        nb, nbb = lone.pop(), G[("batched", l)][1]
        # below the caps (two workgroups per CU lone, one batched: 512 / 256 on an MI355X) the grid is exact
        if _want_nb(npx, False) <= 128:
            assert nb == _want_nb(npx, False), (l, nb)
        else:
            assert 128 < nb <= _want_nb(npx, False), (l, nb)
        assert nbb == _want_nb(npx, True), (l, nbb)
    with pytest.raises(RuntimeError):   # occlusion variants run one alignment per launch
        R._check(R.lib().r360_icp_pass_grid(ctx.h, bank(name, "room", True)[1].h, 0, 1, 1, None, None), "pass_grid")


def test_pass_form_table_coverage(ctx, bank):
    """Over the whole table: every product form at two geometries or more; workgroup counts of 1, of 2..15 (fewer
    than ticket groups), above 16 and no multiple of 16 (a ragged last round of the group reduction); one lone grid
    with fewer threads than pixels (grid-stride, chunk counts 1 and 2)."""
    seen = {}
    nbs, strided = set(), []
    for name, (rows, cols, n) in GEOMS.items():
        G = _grids(ctx, bank, name)
        for (mode, l), (pf, nb) in G.items():
            seen.setdefault(pf, set()).add(name)
            nbs.add(nb)
            if mode != "batched" and nb * TPB < (rows >> l) * (cols >> l):
                strided.append((name, l, nb))
    for pf in (6, 5, 8, 9, 3, 0):
        assert len(seen.get(pf, ())) >= 2, (pf, seen.get(pf))
    assert set(seen) == {6, 5, 8, 9, 3, 0}
    assert 1 in nbs
    assert any(2 <= nb < TICKET_GROUPS for nb in nbs)
    assert any(nb > TICKET_GROUPS and nb % TICKET_GROUPS for nb in nbs)
    assert strided, "no lone grid strides"
    # the capped grid's waves take one chunk or two: 2 * nb * 256 >= npx > nb * 256
    name, l, nb = strided[0]
    npx = (GEOMS[name][0] >> l) * (GEOMS[name][1] >> l)
    assert nb * TPB < npx <= 2 * nb * TPB and npx % (nb * TPB) != 0


def _occ_check(H, g, e, nv, nvis, Hr, gr, er, nvr, nvisr):
    """The bars of test_gpu_occlusion.test_occlusion_pass_parity."""
    assert (nv, nvis) == (nvr, nvisr), (nv, nvr, nvis, nvisr)
    if np.isnan(e) or np.isnan(er):
        assert np.isnan(e) and np.isnan(er), (e, er)
    else:
        assert abs(e - er) <= 1e-6 * abs(er), (e, er)
    sH = max(np.abs(Hr).max(), 1e-30)
    assert np.abs(H - Hr).max() <= 1e-5 * sH
    scale = np.sqrt(np.abs(np.diag(Hr)) * sH) + 1e-12
    assert (np.abs(g - gr) <= 1e-5 * scale).all(), (g - gr, scale)


def _check_pass(got, ref, occ, npx, what):
    """None, or the case and its figures where a bar is missed."""
    H, g, e, nv, nvis = got
    Hr, gr, er, nvr, nvisr = ref
    try:
        if occ == 0:
            icp_check(H, g, e, nv, nvis, Hr, gr, er, nvr, nvisr, npx)
            if nvr == 0:
                assert e == 0.0
        else:
            _occ_check(H, g, e, nv, nvis, Hr, gr, er, nvr, nvisr)
        if nvisr == 0:   # nothing in view: exactly nothing summed
            assert not H.any() and not g.any()
    except AssertionError:
        sH = max(np.abs(Hr).max(), 1e-300)
        sg = max(np.sqrt(np.abs(np.diag(Hr)).max() * (er if occ == 0 else sH)), 1e-300)
        return (f"{what}: counts {(nv, nvis)} vs {(nvr, nvisr)}, dH {np.abs(H - Hr).max() / sH:.2e}, "
                f"dg {np.abs(g - gr).max() / sg:.2e}, de {abs(e - er) / max(abs(er), 1e-300):.2e} ({e!r} vs {er!r})")
    return None


@pytest.mark.parametrize("name,kind,l", PARITY, ids=[f"{n}-{k}-L{l}" for n, k, l in PARITY])
def test_pass_parity_every_form(ctx, bank, name, kind, l):
    """Every cost function, occlusion variant and both poses at one level: the lone pass over compacted frames (PF 5;
    PF 3 / PF 0 with occlusion), the lone pass over streamed frames (PF 6 / 8 / 9, PF 5 where no image form exists) and
    the batched grid (r360_icp_eval_batch, one job) over both, against the oracle's errorPhotoICP_sphere(Occ) +
    calcHessGrad_sphere(Occ) on the oracle's pyramid of the same images.  No level is skipped: where the oracle
    counts no valid pixel the GPU's squared error is exactly 0, where it sees none its H and g are.  The room pair's
    levels of at least 8 rows and 32 columns are not vacuous (the oracle's counts, not the GPU's).

    Found with this test (MI355X): with PF 5's lean transform at every size, the squared error at the second pose missed
    its 1e-6 bar on the two smallest noise levels that still hold valid pixels, the same figure in every PF 5 run of
    them (lone and batched, compacted and streamed frames), counts exact, H within 2.7e-7 and g within 7.2e-7:
      64x384 noise level 4 (4x24), depth cost, 11 valid:  e2 0.4036045267 vs 0.4036038541, 1.67e-6 of it
      64x384 noise level 4, photo + depth cost, 4 valid:   e2 0.1765083745 vs 0.1765081063, 1.52e-6
      80x576 noise level 4 (5x36), depth cost, 27 valid:  e2 1.7809504024 vs 1.7809470569, 1.88e-6
    Not a summation-order effect and not a shape fault: a CPU restatement of the depth-cost pass with the oracle's float
    terms gives the oracle's sum to 4e-8 / 8e-8; with the lean terms (p' by fused multiply-adds, |p'| = d2 rsq(d2))
    it gives 1.62e-6 / 1.31e-6.  The contracted transform moves |p'| of one pixel by an ulp; on these levels that
    pixel carries 58 % / 21 % of the sum and the depth residual T - |p'| (a tenth of |p'|) magnifies the ulp; a
    correctly rounded root alone still leaves 1.30e-6 / 1.08e-6.  PF 5 now takes the reference's p' and |p'| below
    512 valid source points (R360_EXACT_BELOW, icp_kernels.hip), and every case is within its
    bars."""
    rows, cols, n = GEOMS[name]
    regs = {c: _reg(ctx, name, *bank(name, kind, c)) for c in (True, False)}
    npx = (rows >> l) * (cols >> l)
    misses = []
    for method in (0, 1, 2):
        for pi, P in enumerate(POSES):
            for occ in (0, 1, 2):
                ref = oracle_pass(name, kind, l, method, pi, occ)
                if kind != "noise" and (rows >> l) >= 8 and (cols >> l) >= 32:
                    assert ref[3] >= 64 and ref[4] >= 100, (method, pi, occ, ref[3], ref[4])
                for compact, reg in regs.items():
                    what = (method, pi, occ, "compacted" if compact else "streamed")
                    got = reg.eval(l, P, method) if occ == 0 else reg.eval_occ(l, P, method, occ)
                    misses.append(_check_pass(got, ref, occ, npx, what))
                    if occ == 0:
                        Hb, gb, eb, nvb, nvisb = R.align_eval_batch(ctx, [(reg.trg, reg.src)], l, [P], method,
                                                                    _prm(name))
                        misses.append(_check_pass((Hb[0], gb[0], eb[0], int(nvb[0]), int(nvisb[0])), ref, 0, npx,
                                                  what + ("batched",)))
    misses = [m for m in misses if m]
    assert not misses, "\n".join(misses)


def _filler_pose(k):
    rng = np.random.default_rng(100 + k)
    return O.exp_se3(rng.normal(scale=[0.03, 0.03, 0.03, 0.01, 0.01, 0.01]))


@pytest.mark.parametrize("name", ["64x384", "52x416", "20x72"])
def test_batched_pass_is_batch_invariant(ctx, bank, name):
    """A job's batched sums are bit-identical alone, among 3 and among 16 jobs, and in the first, a middle and the
    last slot, whatever the other jobs are (other pairs: the noise spheres and the room pair reversed, each at another
    pose; compacted and streamed frames mixed); its counts are the lone pass's."""
    n = GEOMS[name][2]
    t, s = bank(name, "room", False)
    others = [bank(name, "noise", True), (s, t), bank(name, "noise", False), bank(name, "room", True)[::-1]]
    lone = _reg(ctx, name, t, s)
    P = POSES[1]
    for l in range(n):
        first = R.align_eval_batch(ctx, [(t, s)], l, [P], R.PHOTO_DEPTH, _prm(name))
        first = tuple(a[0] for a in first)
        _, _, _, nv, nvis = lone.eval(l, P, R.PHOTO_DEPTH)
        assert (int(first[3]), int(first[4])) == (nv, nvis), l
        for nj, slots in ((3, (0, 1, 2)), (R.MAX_BATCH_ALIGN, (0, 7, R.MAX_BATCH_ALIGN - 1))):
            for slot in slots:
                pairs = [others[(k + slot) % len(others)] for k in range(nj)]
                poses = [_filler_pose(k + slot) for k in range(nj)]
                pairs[slot], poses[slot] = (t, s), P
                out = R.align_eval_batch(ctx, pairs, l, poses, R.PHOTO_DEPTH, _prm(name))
                for a, b in zip(first, out):
                    assert np.array_equal(np.asarray(a), np.asarray(b[slot])), (l, nj, slot)
                # the other jobs ran their own pairs and poses (a level with nothing in view sums to zero for all)
                assert not first[0].any() or any(not np.array_equal(out[0][k], out[0][slot])
                                                 for k in range(nj) if k != slot), (l, nj, slot)
    with pytest.raises(RuntimeError):
        R.align_eval_batch(ctx, [(t, s)] * (R.MAX_BATCH_ALIGN + 1), 0, [P] * (R.MAX_BATCH_ALIGN + 1), R.PHOTO_DEPTH,
                           _prm(name))
    # refused while a batched alignment is pending on the context (it would overwrite the batch's states)
    p = _prm(name)
    init = np.ascontiguousarray(R._mat16(np.eye(4)), np.float32)
    trg, src = (R.C.c_void_p * 1)(t.h), (R.C.c_void_p * 1)(s.h)
    R._check(R.lib().r360_align360_batch_async(ctx.h, 1, trg, src, R._fptr(init), R.PHOTO_DEPTH, R.C.byref(p)), "async")
    with pytest.raises(RuntimeError):
        R.align_eval_batch(ctx, [(t, s)], 0, [P], R.PHOTO_DEPTH, _prm(name))
    assert R._check(R.lib().r360_align360_batch_result(ctx.h, None, None, None, None), "result") >= 0
    again = R.align_eval_batch(ctx, [(t, s)], n - 1, [P], R.PHOTO_DEPTH, _prm(name))
    assert all(np.array_equal(np.asarray(a), np.asarray(b[0])) for a, b in zip(first, again))


def test_buffers_are_reused_across_geometries(bank):
    """One context through 20x72, 130x1040, 20x72 again, 64x384 and the first two once more, batched and lone at
    every level: the batch buffers and the deferred queues grow with the larger sphere (ensure_batch, ensure_defer)
    and are then reused by grids of another size, as are the ticket counters; every repeat is bit-identical to the
    geometry's first run."""
    c = R.Context(0)
    first = {}
    for name, nj in (("20x72", 1), ("130x1040", 3), ("20x72", 3), ("64x384", 2), ("130x1040", 1), ("20x72", 1),
                     ("64x384", 3)):
        t, s = bank(name, "room", False)
        tn, sn = bank(name, "noise", True)
        reg, regn = _reg(c, name, t, s), _reg(c, name, tn, sn)
        for l in range(GEOMS[name][2]):
            pairs = [(t, s), (tn, sn), (s, t)][:nj]
            poses = [POSES[1], POSES[0], _filler_pose(l)][:nj]
            out = R.align_eval_batch(c, pairs, l, poses, R.PHOTO_DEPTH, _prm(name))
            got = [tuple(np.asarray(a[0]).copy() for a in out)]
            got.append(reg.eval(l, POSES[1], R.PHOTO_DEPTH))
            got.append(regn.eval(l, POSES[1], R.DEPTH_CONSISTENCY))
            got.append(reg.eval_occ(l, POSES[1], R.PHOTO_DEPTH, 2))
            if (name, l) not in first:
                first[(name, l)] = got
                continue
            for a, b in zip(first[(name, l)], got):
                for x, y in zip(a, b):
                    assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), (name, l, nj)
    c.close()


# ---------------------------------------------------------------- whole alignments
ALIGN = {"64x384": 5, "52x416": 3, "20x72": 2}   # geometry: n_pyr


def _params(n_pyr, fixed):
    p = R.IcpParams.default()
    p.n_pyr = n_pyr
    p.std_dev_photo = np.float32(3.0 / 255)
    p.fixed_iters_level0 = fixed
    return p


@functools.lru_cache(maxsize=None)
def oracle_align(name, fixed, occ):
    (tb, td), (sb, sd) = images(name, "room")
    p = O.IcpParams.default(n_pyr=ALIGN[name], std_dev_photo=np.float32(3.0 / 255), fixed_iters_level0=fixed)
    rc, pose, H, g, st = O.align360(tb, td, sb, sd, None, O.PHOTO_DEPTH, p, occlusion=occ)
    return rc, pose, list(st.iters)[:ALIGN[name]]


def _lone(c, name, t, s, p, occ=0):
    reg = _reg(c, name, t, s)
    reg.params = p
    rc = reg.alignFrames360(np.eye(4), R.PHOTO_DEPTH, occ)
    return dict(rc=rc, pose=reg.getOptimalPose().copy(), H=reg.getHessian().copy(), g=reg.getGradient().copy(),
                iters=list(reg.stats.iters), evals=list(reg.stats.evals), persistent=reg.stats.persistent)


def _vs_oracle(got_rc, got_pose, got_iters, ref, what):
    rc, pose, iters = ref
    assert got_rc == rc, what
    dr, dt = O.rot_angle(got_pose, pose), float(np.linalg.norm(np.asarray(got_pose)[:3, 3] - pose[:3, 3]))
    assert dr <= ROT_TOL and dt <= TRANS_TOL, (what, dr, dt)
    n = len(iters)
    # equal Gauss-Newton decisions, or one at a rounding edge flipped (test_gpu_batch_align._close_to)
    assert all(abs(a - b) <= 1 for a, b in zip(got_iters[:n], iters)), (what, got_iters[:n], iters)


def _same_bits(a, b, what):
    for k in ("pose", "H", "g"):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert a["rc"] == b["rc"] and a["iters"] == b["iters"] and a["evals"] == b["evals"], what


@pytest.mark.parametrize("fixed", [0, 6])
@pytest.mark.parametrize("name", list(ALIGN))
def test_whole_alignments(ctx, bank, name, fixed):
    """alignFrames360 (PHOTO_DEPTH, sigma 3/255) of the room pair through every path: lone over compacted and over
    streamed frames, lone with persistent level launches, lone with occlusion 1 / 2, batched alone and in every slot
    of a batch of three beside the noise pair.  Each against the oracle's alignFrames360 (status, north-star pose
    bar, iteration counts within one flip); persistent equals per-pass and a batch of one equals a batch of three,
    bit for bit.  The oracle's own result is not vacuous: on 64x384 and 52x416 it iterates at least twice on two
    levels and recovers the displacement between the two eyes within 5 mm."""
    n_pyr = ALIGN[name]
    ref = oracle_align(name, fixed, 0)
    if name != "20x72":
        assert sum(1 for k in ref[2] if k >= 2) >= 2, ref[2]
        assert np.linalg.norm(ref[1][:3, 3] - np.array(ROOM_MOTION)) <= 5e-3, ref[1][:3, 3]
    full, lean = bank(name, "room", True), bank(name, "room", False)
    a = _lone(ctx, name, *full, _params(n_pyr, fixed))
    _vs_oracle(a["rc"], a["pose"], a["iters"], ref, "lone compacted")
    b = _lone(ctx, name, *lean, _params(n_pyr, fixed))
    _vs_oracle(b["rc"], b["pose"], b["iters"], ref, "lone streamed")
    pc = R.Context(0)
    pc.persistent_levels(True)
    c = _lone(pc, name, *full, _params(n_pyr, fixed))
    pc.close()
    assert c["persistent"] == 1 and a["persistent"] == 0
    _same_bits(a, c, "persistent vs per-pass")
    for occ in (1, 2):
        o = _lone(ctx, name, *full, _params(n_pyr, fixed), occ)
        _vs_oracle(o["rc"], o["pose"], o["iters"], oracle_align(name, fixed, occ), f"lone occlusion {occ}")
    noise = bank(name, "noise", False)
    for frames, what in ((lean, "batched streamed"), (full, "batched compacted")):
        poses, H, g, st, ill = R.align360_batch(ctx, [frames], None, R.PHOTO_DEPTH, _params(n_pyr, fixed))
        one = dict(rc=int(bool(st[0].illposed)), pose=poses[0], H=H[0], g=g[0], iters=list(st[0].iters),
                   evals=list(st[0].evals))
        assert ill == one["rc"]
        _vs_oracle(one["rc"], one["pose"], one["iters"], ref, what)
        for slot in range(3):
            pairs = [noise, noise[::-1], noise]
            pairs[slot] = frames
            poses, H, g, st, ill = R.align360_batch(ctx, pairs, None, R.PHOTO_DEPTH, _params(n_pyr, fixed))
            got = dict(rc=int(bool(st[slot].illposed)), pose=poses[slot], H=H[slot], g=g[slot],
                       iters=list(st[slot].iters), evals=list(st[slot].evals))
            _same_bits(one, got, (what, "slot", slot))
