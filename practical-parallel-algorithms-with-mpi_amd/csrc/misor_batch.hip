// misor_batch.hip -- the batched solve of include/misor.h (misor_batch_*):
// nbatch independent problems of one shape, each in the single grid's padded
// layout, solved by ONE launch of rb_solve_batch_kernel (sor_kernels.hip) --
// one workgroup per member, p in LDS, the body rb_solve_small_kernel runs.
//
// Per member the device holds {coef, DevState} (BatchMember): the array goes
// up before the launch and comes back after it, one copy each way per solve.
// A member the kernel stopped near its threshold (DevState::near; its p left
// untouched) is finished by the library's single-grid path on one internal
// misor_grid of the batch's shape (grid_adopt, misor_solve_rb: the re-run up to
// the near iteration and the exact tail of misor_solve.hip), so it ends with
// the bits misor_solve_rb gives for it alone.
//
// Every argument check precedes the first HIP call, and the device is first
// touched by the first call that moves or computes data (ensure_device).

#include "misor_grid.h"

struct misor_batch {
    misor_batch_desc desc{};
    int device = -1;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool ready = false;  // device chosen, stream and fields there
    long long pitch = 0, rows = 0, elems = 0;  // of one member
    double* p = nullptr;    // nbatch members, elems doubles apart
    double* rhs = nullptr;
    std::vector<double> omega, eps;
    std::vector<int> itermax;
    BatchMember* members = nullptr;        // device
    std::vector<BatchMember> members_host;
    int near_exp = 10;  // MISOR_TUNE_NEAR_BAND, as misor_grid
    double near_rel = 1e-10;
    misor_grid* scratch = nullptr;  // finishes the members stopped near the threshold
};

namespace {

double* member_origin(const misor_batch* b, double* base, int m) {
    return base + (long long)m * b->elems + (long long)kYOff * b->pitch + kXOff;  // cell (0,0)
}

int ensure_device(misor_batch* b) {
    if (b->ready) {
        HIPCHK(hipSetDevice(b->device));
        return MISOR_OK;
    }
    if (b->desc.device >= 0) {
        b->device = b->desc.device;
        HIPCHK(hipSetDevice(b->device));
    } else {
        HIPCHK(hipGetDevice(&b->device));
    }
    if (!b->stream) {
        HIPCHK(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
        b->own_stream = true;
    }
    const size_t bytes = (size_t)b->elems * b->desc.nbatch * sizeof(double);
    if (hipMalloc(&b->p, bytes) != hipSuccess || hipMalloc(&b->rhs, bytes) != hipSuccess ||
        hipMalloc(&b->members, sizeof(BatchMember) * b->desc.nbatch) != hipSuccess) {
        (void)hipFree(b->p);
        (void)hipFree(b->rhs);
        (void)hipFree(b->members);
        b->p = b->rhs = nullptr;
        b->members = nullptr;
        return fail(MISOR_ENOMEM, "hipMalloc of %d members of %lld doubles failed",
                    b->desc.nbatch, 2 * b->elems);
    }
    // padding cells are zero, as in a grid
    HIPCHK(hipMemsetAsync(b->p, 0, bytes, b->stream));
    HIPCHK(hipMemsetAsync(b->rhs, 0, bytes, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    b->ready = true;
    return MISOR_OK;
}

// the checks of upload / download (no HIP call before them)
int check_transfer(const misor_batch* b, int field, int member, const void* host,
                   const char* what) {
    if (!b || !host) return fail(MISOR_EINVAL, "%s: null argument", what);
    if (field != MISOR_P && field != MISOR_RHS)
        return fail(MISOR_EINVAL, "%s: a batch holds MISOR_P and MISOR_RHS only (field %d)", what,
                    field);
    if (member < -1 || member >= b->desc.nbatch)
        return fail(MISOR_EINVAL, "%s: member %d outside [0, %d) (-1: all)", what, member,
                    b->desc.nbatch);
    return MISOR_OK;
}

// The member the kernel stopped near its threshold, through the single grid's
// own path from the member's untouched p.
int finish_near(misor_batch* b, int m, int* iters, double* res) {
    if (!b->scratch) {
        misor_desc d{};
        d.imax = b->desc.imax;
        d.jmax = b->desc.jmax;
        d.dx = b->desc.dx;
        d.dy = b->desc.dy;
        d.omega = 1.0;
        d.variant = b->desc.variant;
        d.device = b->device;
        d.nranks = 1;
        MISOR_TRY(misor_create(&b->scratch, &d));
    }
    misor_grid* g = b->scratch;
    MISOR_TRY(misor_set_tuning(g, MISOR_TUNE_NEAR_BAND, b->near_exp));
    double* pm = b->p + (long long)m * b->elems;
    MISOR_TRY(grid_adopt(g, pm, b->rhs + (long long)m * b->elems, b->omega[m], b->eps[m],
                         b->itermax[m]));
    MISOR_TRY(misor_solve_rb(g, iters, res));
    HIPCHK(hipMemcpyAsync(pm, pbuf(g, g->cur), (size_t)b->elems * sizeof(double),
                          hipMemcpyDeviceToDevice, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return MISOR_OK;
}

}  // namespace

int misor_batch_create(misor_batch** out, const misor_batch_desc* d) {
    if (!out || !d) return fail(MISOR_EINVAL, "null argument");
    *out = nullptr;
    if (d->imax < 1 || d->jmax < 1) return fail(MISOR_EINVAL, "imax, jmax must be >= 1");
    if (!(d->dx > 0) || !(d->dy > 0)) return fail(MISOR_EINVAL, "dx, dy must be > 0");
    if (d->nbatch < 1) return fail(MISOR_EINVAL, "nbatch must be >= 1");
    if (d->variant != MISOR_SOLVE_RB && d->variant != MISOR_SOLVE_RBA)
        return fail(MISOR_EINVAL, "variant must be MISOR_SOLVE_RB or MISOR_SOLVE_RBA");
    if (!small_solve_fits(d->imax, d->jmax))
        return fail(MISOR_EINVAL,
                    "a batch holds LDS-resident problems only (up to 128^2 cells); %d x %d does "
                    "not fit: use misor_create for it",
                    d->imax, d->jmax);
    misor_batch* b = new misor_batch();
    b->desc = *d;
    b->pitch = layout_pitch(d->imax);
    b->rows = layout_rows(d->jmax);
    b->elems = b->pitch * b->rows;
    b->omega.assign(d->nbatch, 1.0);
    b->eps.assign(d->nbatch, 0.0);
    b->itermax.assign(d->nbatch, 0);
    b->members_host.resize(d->nbatch);
    *out = b;
    return MISOR_OK;
}

void misor_batch_destroy(misor_batch* b) {
    if (!b) return;
    if (b->ready) (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    misor_destroy(b->scratch);
    (void)hipFree(b->p);
    (void)hipFree(b->rhs);
    (void)hipFree(b->members);
    if (b->own_stream && b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

int misor_batch_set_params(misor_batch* b, const double* omega, const double* eps,
                           const int* itermax) {
    if (!b) return fail(MISOR_EINVAL, "null batch");
    const int n = b->desc.nbatch;
    if (omega) b->omega.assign(omega, omega + n);
    if (eps) b->eps.assign(eps, eps + n);
    if (itermax) b->itermax.assign(itermax, itermax + n);
    return MISOR_OK;
}

int misor_batch_upload(misor_batch* b, int field, int member, const double* host) {
    MISOR_TRY(check_transfer(b, field, member, host, "misor_batch_upload"));
    MISOR_TRY(ensure_device(b));
    const size_t w = (size_t)(b->desc.imax + 2) * sizeof(double);
    const size_t h = (size_t)(b->desc.jmax + 2);
    double* base = field == MISOR_P ? b->p : b->rhs;
    const int m0 = member < 0 ? 0 : member, m1 = member < 0 ? b->desc.nbatch : member + 1;
    for (int m = m0; m < m1; ++m)
        HIPCHK(hipMemcpy2DAsync(member_origin(b, base, m), b->pitch * sizeof(double),
                                host + (size_t)(m - m0) * (w / sizeof(double)) * h, w, w, h,
                                hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return MISOR_OK;
}

int misor_batch_download(misor_batch* b, int field, int member, double* host) {
    MISOR_TRY(check_transfer(b, field, member, host, "misor_batch_download"));
    MISOR_TRY(ensure_device(b));
    const size_t w = (size_t)(b->desc.imax + 2) * sizeof(double);
    const size_t h = (size_t)(b->desc.jmax + 2);
    double* base = field == MISOR_P ? b->p : b->rhs;
    const int m0 = member < 0 ? 0 : member, m1 = member < 0 ? b->desc.nbatch : member + 1;
    for (int m = m0; m < m1; ++m)
        HIPCHK(hipMemcpy2DAsync(host + (size_t)(m - m0) * (w / sizeof(double)) * h, w,
                                member_origin(b, base, m), b->pitch * sizeof(double), w, h,
                                hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return MISOR_OK;
}

int misor_batch_poisson_init(misor_batch* b, double xlength, double ylength, int problem) {
    if (!b) return fail(MISOR_EINVAL, "null batch");
    MISOR_TRY(ensure_device(b));
    const int ni = b->desc.imax, nj = b->desc.jmax;
    misor_local loc{};  // the whole domain: one rank
    loc.ni = ni;
    loc.nj = nj;
    const std::vector<double> host = poisson_tables(loc, ni, nj, xlength, ylength);
    double* tab = nullptr;
    HIPCHK(hipMalloc(&tab, host.size() * sizeof(double)));
    if (hipMemcpyAsync(tab, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice,
                       b->stream) != hipSuccess) {
        (void)hipFree(tab);
        return fail(MISOR_EHIP, "copy of the sine tables failed");
    }
    for (int m = 0; m < b->desc.nbatch; ++m)
        launch_poisson_init(b->stream, b->p + (long long)m * b->elems,
                            b->rhs + (long long)m * b->elems, tab, tab + 2 * (ni + 2),
                            tab + (ni + 2), ni, nj, b->pitch, problem);
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(b->stream);
    (void)hipFree(tab);
    HIPCHK(e1);
    HIPCHK(e2);
    return MISOR_OK;
}

int misor_batch_solve_rb(misor_batch* b, int* iters, double* res) {
    if (!b) return fail(MISOR_EINVAL, "null batch");
    MISOR_TRY(ensure_device(b));
    const int n = b->desc.nbatch, ni = b->desc.imax, nj = b->desc.jmax;
    // misor_create has no grid with a side of 1: nothing to agree with, no band
    const bool banded = ni >= 2 && nj >= 2;
    SorConsts sc{};
    for (int m = 0; m < n; ++m) {
        sc = sor_consts(b->desc.dx, b->desc.dy, b->omega[m], b->desc.variant);
        BatchMember& mb = b->members_host[m];
        mb.coef = sc.coef;
        DevState s{};  // solveRB's start: no iteration done, res = 1.0 (solver.c:196)
        s.res = 1.0;
        s.epssq = b->eps[m] * b->eps[m];
        s.itermax = b->itermax[m];
        s.nband = banded ? near_band_abs(b->near_rel, s.epssq) : -1.0;
        mb.st = s;
    }
    const double cells = (double)ni * (double)nj;
    const size_t bytes = sizeof(BatchMember) * (size_t)n;
    HIPCHK(hipMemcpyAsync(b->members, b->members_host.data(), bytes, hipMemcpyHostToDevice,
                          b->stream));
    launch_solve_batch(b->stream, b->p, b->rhs, b->elems, n, ni, nj, b->pitch, sc.idx2, sc.idy2,
                       cells, b->members);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(b->members_host.data(), b->members, bytes, hipMemcpyDeviceToHost,
                          b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    for (int m = 0; m < n; ++m) {
        const DevState& s = b->members_host[m].st;
        int it = s.it;
        double r = s.res;
        if (s.near) MISOR_TRY(finish_near(b, m, &it, &r));
        if (iters) iters[m] = it;
        if (res) res[m] = r;
    }
    return MISOR_OK;
}

int misor_batch_set_stream(misor_batch* b, void* s) {
    if (!b) return fail(MISOR_EINVAL, "null batch");
    if (b->ready) HIPCHK(hipSetDevice(b->device));
    if (b->stream) HIPCHK(hipStreamSynchronize(b->stream));
    if (b->own_stream) HIPCHK(hipStreamDestroy(b->stream));
    b->stream = (hipStream_t)s;  // NULL: an own stream, made at the next device call
    b->own_stream = false;
    if (!s && b->ready) {
        HIPCHK(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
        b->own_stream = true;
    }
    return MISOR_OK;
}

int misor_batch_set_tuning(misor_batch* b, int key, int value) {
    if (!b) return fail(MISOR_EINVAL, "null batch");
    if (key != MISOR_TUNE_NEAR_BAND)
        return fail(MISOR_EINVAL, "a batch has MISOR_TUNE_NEAR_BAND only (key %d)", key);
    b->near_exp = value;
    b->near_rel = near_band_rel(value);
    return MISOR_OK;
}

int misor_batch_get_tuning(const misor_batch* b, int key, int* value) {
    if (!b || !value) return fail(MISOR_EINVAL, "null argument");
    if (key != MISOR_TUNE_NEAR_BAND)
        return fail(MISOR_EINVAL, "a batch has MISOR_TUNE_NEAR_BAND only (key %d)", key);
    *value = b->near_exp;
    return MISOR_OK;
}
