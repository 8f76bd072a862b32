// handles.cpp — the memory of the handles whose buffers are sized once at creation: r360_calib, r360_frame and the
// frame's PlaneBufs.  Which buffers, how many items, the events, the initial memset or memcpy, and the release of all
// of it when a step fails.  Nothing here launches a kernel or needs more of HIP than the allocation, copy and event
// calls, so tests/host/devmem_check.cpp builds this file against its mock runtime and fails every call in turn.
#include <cmath>
#include <cstring>

#include "../r360_internal.h"

// ------------------------------------------------------------------ Calib360
namespace {

int upload_floats(BufSet& mem, float*& view, const std::vector<float>& h) {
    if (mem.take(view, h.size() ? h.size() : 1)) return -1;
    R360_HIP(hipMemcpy(view, h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice));
    return 0;
}

int replace_floats(DevBuf<float>& own, float*& view, const std::vector<float>& h) {
    view = nullptr;
    own.reset();   // release, then allocate: see r360_calib::upload_clams
    if (own.reserve(nullptr, h.size() ? h.size() : 1)) return -1;
    view = own.get();
    R360_HIP(hipMemcpy(view, h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice));
    return 0;
}

}  // namespace

// Trigonometric tables with the reference's exact float expressions:
//   stitchImage (Frame360.h:1104-1129) and the alignFrames360 LUT (RegisterPhotoICP.h:4555-4569).
// (The kernels' comments know this routine by its former name, calib_build_tables.)
int r360_calib::alloc(int want_rows, int want_cols) {
    for (int k = 0; k < 8; ++k)
        for (int i = 0; i < 16; ++i) rt[k][i] = rt_inv[k][i] = (i % 5 == 0) ? 1.f : 0.f;
    if (rows) {   // a sphere-only calibration has no sensors: no device extrinsics, no stitch tables
        if (mem.take(d_rt_inv, 128)) return -1;
        R360_HIP(hipMemcpy(d_rt_inv, rt_inv, sizeof(float) * 128, hipMemcpyHostToDevice));
        if (mem.take(d_rt, 128)) return -1;
        R360_HIP(hipMemcpy(d_rt, rt, sizeof(float) * 128, hipMemcpyHostToDevice));
    }
    const int W = want_cols ? want_cols : rows * 8;
    const int H = want_rows ? want_rows : (int)(W * 0.5 * 60.0 / 180);
    sph_rows = H; sph_cols = W;
    if (rows) {
        const float offsetPhi = H / 2 - 0.5;
        const float offsetTheta = -rows * 15 / 2 + 0.5;
        const float angle_pixel = 2 * R360_PI / W;
        std::vector<float> sp(H), cp(H), st(W), ct(W);
        for (int r = 0; r < H; ++r) { float phi_i = (offsetPhi - r) * angle_pixel; sp[r] = std::sin(phi_i); cp[r] = std::cos(phi_i); }
        for (int col = 0; col < W; ++col) { float th = (col + offsetTheta) * angle_pixel; st[col] = std::sin(th); ct[col] = std::cos(th); }
        if (upload_floats(mem, d_st_sinphi, sp) || upload_floats(mem, d_st_cosphi, cp) || upload_floats(mem, d_st_sinth, st) ||
            upload_floats(mem, d_st_costh, ct))
            return -1;
    }
    // pyramid levels of the sphere
    int R = H, C = W, nl = 0;
    for (; nl < R360_MAX_PYR; ++nl) {
        if (R < 2 || C < 8 || (C % 4) != 0) break;
        const float angle_res = 2 * R360_PI / C;
        const float half_nRows = 0.5 * R - 0.5;
        std::vector<float> a(R), b(R), s(C), t(C);
        for (int cc = 0; cc < C; ++cc) { float theta = cc * angle_res; s[cc] = std::sin(theta); t[cc] = std::cos(theta); }
        for (int r = 0; r < R; ++r) { float phi = (half_nRows - r) * angle_res; a[r] = std::sin(phi); b[r] = std::cos(phi); }
        LevelTrig& L = trig[nl];
        if (upload_floats(mem, L.sinphi, a) || upload_floats(mem, L.cosphi, b) || upload_floats(mem, L.sinth, s) ||
            upload_floats(mem, L.costh, t))
            return -1;
        if ((R % 2) || (C % 2)) { ++nl; break; }
        R /= 2; C /= 2;
    }
    n_levels = nl;
    return 0;
}

int r360_calib::upload_clams(const std::vector<float>& mult, const std::vector<float>& counts) {
    return replace_floats(clams_mult, clams.d_mult, mult) || replace_floats(clams_counts, clams.d_counts, counts) ? -1 : 0;
}

int calib_new(r360_ctx* ctx, int rows, int cols, int sph_rows, int sph_cols, r360_calib** out) {
    R360_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<r360_calib> c(new r360_calib);
    c->ctx = ctx; c->rows = rows; c->cols = cols;
    if (c->alloc(sph_rows, sph_cols)) return -1;
    *out = c.release();
    return 0;
}

// ------------------------------------------------------------------ Frame360
int r360_frame::alloc() {
    rows = calib->rows; cols = calib->cols;
    sph_rows = calib->sph_rows; sph_cols = calib->sph_cols;
    n_levels = calib->n_levels;
    const size_t ns = (size_t)8 * rows * cols, nsph = (size_t)sph_rows * sph_cols;
    if (ns) {                        // a sphere-only frame (r360_calib_create_sphere) has no sensor images
        if (mem.take(d_bgr, ns * 3) || mem.take(d_depth, ns) || mem.take(d_depth_m, ns)) return -1;
    }
    if (mem.take(d_sph_bgr, nsph * 3) || mem.take(d_sph_depth, nsph)) return -1;
    int R = sph_rows, C = sph_cols;
    for (int l = 0; l < n_levels; ++l) {
        LevelBufs& L = lv[l];
        L.rows = R; L.cols = C;
        const size_t n = (size_t)R * C;
        if (mem.take(L.p0, n) || mem.take(L.tg, n) || mem.take(L.pts, n) || (l == 0 && mem.take(L.pk, n))) return -1;
        R /= 2; C /= 2;
    }
    src_blocks = (int)((nsph + R360_SRC_BLOCK - 1) / R360_SRC_BLOCK);
    if (mem.take(d_npts, R360_MAX_PYR)) return -1;
    R360_HIP(hipMemsetAsync(d_npts, 0, sizeof(int) * R360_MAX_PYR, ctx->stream));
    if (mem.take(d_src_cnt, R360_MAX_PYR * (size_t)src_blocks)) return -1;
    SrcLevel sl[R360_MAX_PYR];
    for (int l = 0; l < n_levels; ++l) {
        const LevelTrig& T = calib->trig[l];
        sl[l] = SrcLevel{lv[l].p0, lv[l].pts, T.sinphi, T.cosphi, T.sinth, T.costh, lv[l].rows, lv[l].cols};
    }
    if (mem.take(d_src_levels, R360_MAX_PYR)) return -1;
    R360_HIP(hipMemcpy(d_src_levels, sl, sizeof(SrcLevel) * n_levels, hipMemcpyHostToDevice));
    R360_HIP(hipEventCreateWithFlags(&bgr_ev, hipEventDisableTiming));
    return 0;
}

int r360_frame::alloc_sensor_pyramid() {
    if (n_slevels) return 0;
    int R = rows, C = cols, nl = 0;
    while (nl < R360_MAX_PYR) {
        LevelBufs& L = sp[nl];
        L.rows = R; L.cols = C;
        if (sp_mem.take(L.p0, 8 * (size_t)R * C) || sp_mem.take(L.tg, 8 * (size_t)R * C)) {
            sp_mem.release();
            for (int l = 0; l <= nl; ++l) sp[l] = LevelBufs();
            return -1;
        }
        ++nl;
        if ((R & 1) || (C & 1) || R < 8 || C < 8) break;   // cv::pyrDown halves exactly only even sizes
        R /= 2; C /= 2;
    }
    n_slevels = nl;
    return 0;
}

r360_frame::~r360_frame() {
    if (bgr_ev) (void)hipEventDestroy(bgr_ev);
    delete sphere_cloud;
}

int frame_new(r360_ctx* ctx, const r360_calib* calib, r360_frame** out) {
    R360_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<r360_frame> f(new r360_frame);
    f->ctx = ctx; f->calib = calib;
    if (f->alloc()) return -1;
    *out = f.release();
    return 0;
}

// ------------------------------------------------------------------ the frame's plane half
int PlaneBufs::alloc(int rows, int cols) {
    if (v.cloud) return 0;
    w = cols / 2;
    h = rows / 2;
    const size_t N = (size_t)w * h, T = 8 * N;
    const long sw = (w - 1) / 10 + 5, sh = (h - 1) / 10 + 5;
    sd_max = 208;
    grid_cells = sw * sh * sd_max;
    const size_t SK = 8 * (size_t)(w + h - 1) * h;   // the wavefront refinement's skewed images [8][h + w - 1][h]
    v.contour_cap = 2 * (long)T;
    v.vox_cap = (long)T;
    auto event = [](hipEvent_t* e, unsigned flags) {
        R360_HIP(hipEventCreateWithFlags(e, flags));
        return 0;
    };
    const bool failed =
        mem.take(v.cloud, T) ||          // [8][h][w] {x, y, z, 0}
        mem.take(v.rgb, T) ||            // {r, g, b, 0}
        mem.take(v.nrm, T) ||            // {nx, ny, nz, d = p.n}
        mem.take(v.dist0, T) ||          // distance-map init (depth-change map)
        mem.take(v.dist, T) ||           // distance map
        mem.take(v.grids, 16 * (size_t)grid_cells) ||   // bilateral grids, 8 x 2 x grid_cells
        mem.take(v.zmm, 16) ||           // per-sensor depth range for the bilateral grid: [8] min, [8] max (ordered ints)
        mem.take(v.parent, T) ||         // union-find parents, then root ranks
        mem.take(v.root, T) ||
        mem.take(v.lab, T) ||            // CCL labels (per-sensor ids, -1 none)
        mem.take(v.labf, T) ||           // labels after refinement
        mem.take(v.cnt, T) ||            // label sizes [8][N]
        mem.take(v.aux, 8 * R360_MAX_BIG) ||             // the large labels' first pixels (plane_seg.hip)
        mem.take(v.chunk, 8 * ((N + 255) / 256)) ||      // per-chunk counts of the numbering kernels
        mem.take(v.gpart, (size_t)R360_GM_COPIES * 8 * R360_MAX_MODELS) ||   // region accumulators (k_gm<true>)
        mem.take(v.nlab, 8) ||
        mem.take(v.big, 8 * R360_MAX_BIG) ||
        mem.take(v.nbig, 8) ||
        mem.take(v.mom, 8 * R360_MAX_BIG) ||             // the large labels' moments
        mem.take(v.models, 8 * R360_MAX_MODELS) ||
        mem.take(v.nmodels, 8) ||
        mem.take(v.state, T) ||          // refinement state [8][N]
        mem.take(v.state2, T) ||         // refinement state after the first sweep
        mem.take(v.rbnd, 8 * (size_t)R360_REFINE_BANDS * w) ||   // banded refinement: each band's assignments into the
        mem.take(v.rflag, 8 * R360_REFINE_BANDS) ||              //   next band's first row, and whether they changed it
        mem.take(v.mask, T) ||           // closeness masks [8][N]
        mem.take(v.rcode, SK) ||         // wavefront refinement, skewed: state | push conditions
        mem.take(v.rmsk, SK) ||          //   closeness masks
        mem.take(v.rf1, SK) ||           //   first sweep's states
        mem.take(v.rf2, SK) ||           //   second sweep's states
        mem.take(v.out, 8 * R360_MAX_MODELS) ||
        // the contour and voxel outputs are written by the kernels straight into pinned host memory (a few hundred KB
        // per frame), so the host assembly needs no second device->host copy
        mem.take_pinned(v.contour, v.contour_cap) ||     // contour points kept by the hull prefilter
        mem.take(v.contour_dev, v.contour_cap) ||        // the traced contours (k_trace -> k_hullpre)
        mem.take_pinned(v.vox, v.vox_cap) ||             // voxel-fallback centroids kept by the hull prefilter
        mem.take(v.vox_dev, v.vox_cap) ||                // all voxel-fallback centroids (k_vox_compact -> k_hullpre)
        event(&done, hipEventDisableTiming | hipEventBlockingSync) ||
        event(&ready, hipEventDisableTiming) ||
        mem.take(v.totals, 4) ||         // [2] pool usage
        mem.take(v.err, 1) ||            // error bits
        mem.take_pinned(v.h_out, 8 * R360_MAX_MODELS) || // pinned host mirrors: the models,
        mem.take_pinned(v.h_nmodels, 16);                //   nmodels [8], then err at [8], totals at (long*)(h_nmodels + 10)
    if (!failed) return 0;
    release();   // the next call starts again
    return -1;
}

void PlaneBufs::release() {
    mem.release();
    if (done) (void)hipEventDestroy(done);
    if (ready) (void)hipEventDestroy(ready);
    done = ready = nullptr;
    v = PlaneDev{};
    w = h = sd_max = 0;
    grid_cells = 0;
    ticket.reset();
    asm_busy = false;
    worker_rc = 0;
    worker_err.clear();
}
