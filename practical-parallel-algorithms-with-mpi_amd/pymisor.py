"""ctypes binding of libmisor (include/misor.h).

This is the Python-side stub of the C ABI: tests/, bench.py and
__graft_entry__.py drive the HIP path through it.  It loads the in-tree
lib/libmisor.so and fails loudly when that library is missing -- there is no
CPU fallback anywhere in the product path.

Host arrays are numpy float64 of shape (nj+2, ni+2): the reference layout
P(i,j) = p[j*(imax+2)+i] (assignment-4/src/solver.c:16) of this rank's block.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.path.join(HERE, "lib", "libmisor.so")
_DEFAULT_LIBPATH = LIBPATH

P, RHS, U, V, F, G = range(6)
NOSLIP, SLIP, OUTFLOW, PERIODIC = 1, 2, 3, 4
PROBLEM_NONE, PROBLEM_DCAVITY, PROBLEM_CANAL = 0, 1, 2
SOLVE_RB, SOLVE_RBA = 0, 1
LEX_A4, LEX_SEQ = 0, 1
(TUNE_SWEEP_VARIANT, TUNE_ROWS_PER_BLOCK, TUNE_XCD_REMAP, TUNE_SMALL_SOLVE, TUNE_OVERLAP,
 TUNE_TSTEPS, TUNE_TB_VARIANT, TUNE_TB_ROWS, TUNE_TB_PERSISTENT, TUNE_NS_FUSE,
 TUNE_FINISH2, TUNE_TB_RESERVE, TUNE_TB_CHAIN, TUNE_NEAR_BAND, TUNE_RES_LITE,
 TUNE_EDGE_STEAL, TUNE_LEX_TILED, TUNE_LEX_TILE_W, TUNE_LEX_TILE_H,
 TUNE_LEX_WGS, TUNE_MG_TAIL) = range(1, 22)
COMM_ID_BYTES = 128
# 3D field ids (misor3_*)
P3, RHS3, U3, V3, W3, F3, G3, H3 = range(8)
TUNE3_SWEEP, TUNE3_ROWS, TUNE3_KCHUNK, TUNE3_FOLD, TUNE3_RHS_AHEAD = 1, 2, 3, 4, 5
TUNE3_RESIDENT = 6  # whole solve in one cooperative launch, p in LDS (when it fits)

_dp = C.POINTER(C.c_double)


class Desc(C.Structure):
    _fields_ = [("imax", C.c_int), ("jmax", C.c_int), ("dx", C.c_double), ("dy", C.c_double),
                ("omega", C.c_double), ("eps", C.c_double), ("itermax", C.c_int),
                ("variant", C.c_int), ("device", C.c_int), ("nranks", C.c_int),
                ("rank", C.c_int), ("dims", C.c_int * 2), ("comm_id", C.c_void_p)]


class NsDesc(C.Structure):
    _fields_ = [("xlength", C.c_double), ("ylength", C.c_double), ("re", C.c_double),
                ("gx", C.c_double), ("gy", C.c_double), ("gamma", C.c_double),
                ("tau", C.c_double), ("bcLeft", C.c_int), ("bcRight", C.c_int),
                ("bcBottom", C.c_int), ("bcTop", C.c_int), ("problem", C.c_int)]


class BatchDesc(C.Structure):
    _fields_ = [("imax", C.c_int), ("jmax", C.c_int), ("dx", C.c_double), ("dy", C.c_double),
                ("nbatch", C.c_int), ("variant", C.c_int), ("device", C.c_int)]


class Local(C.Structure):
    _fields_ = [("ni", C.c_int), ("nj", C.c_int), ("ioff", C.c_int), ("joff", C.c_int),
                ("coords", C.c_int * 2), ("dims", C.c_int * 2), ("neighbours", C.c_int * 4),
                ("pitch", C.c_longlong)]


class Stats(C.Structure):
    _fields_ = [("sweeps", C.c_longlong), ("launches", C.c_longlong), ("sweep_ms", C.c_double),
                ("timed_sweeps", C.c_longlong), ("timed_passes", C.c_longlong),
                ("iters_per_pass", C.c_int), ("tb_variant", C.c_int),
                ("halo_ms", C.c_double), ("halos", C.c_longlong),
                ("allreduce_ms", C.c_double), ("allreduces", C.c_longlong),
                ("chained", C.c_int), ("ns_ms", C.c_double * 3), ("ns_calls", C.c_longlong * 3),
                ("lite_misses", C.c_longlong),
                ("mg_cycles", C.c_int), ("mg_levels", C.c_int),
                ("mg_transfer_ms", C.c_double * 2), ("mg_transfers", C.c_longlong)]


class StatsTail(Stats):
    """misor_stats whole: Stats is its layout up to mg_transfers, kept under that
    name with those fields last; what was appended since follows here (a ctypes
    subclass lays its fields out behind the base's, as C does)"""
    _fields_ = [("mg_tail_levels", C.c_int), ("mg_tail_launches", C.c_longlong),
                ("mg_tail_fallbacks", C.c_longlong), ("mg_tail_ms", C.c_double)]


class StatsDist(StatsTail):
    """misor_stats whole: StatsTail and what was appended after it"""
    _fields_ = [("mg_dist_levels", C.c_int)]


class MgInfo3(C.Structure):
    _fields_ = [("cycles", C.c_int), ("levels", C.c_int), ("transfer_ms", C.c_double * 2),
                ("transfers", C.c_longlong), ("dist_levels", C.c_int)]


class _MgInfo3Dict(dict):
    """Grid3.mg_info(): "dist_levels" is an entry where the last solve kept levels
    distributed and reads as 0 where it did not (misor3_solve_mg, one rank), so
    that the dict of a single-rank solve is what it was before the field existed"""

    def __missing__(self, key):
        if key == "dist_levels":
            return 0
        raise KeyError(key)


class MgParams(C.Structure):
    _fields_ = [("nu1", C.c_int), ("nu2", C.c_int), ("omega_smooth", C.c_double),
                ("coarse_cells", C.c_int), ("omega_coarse", C.c_double),
                ("eps_coarse", C.c_double), ("itermax_coarse", C.c_int),
                ("maxcycles", C.c_int)]


class Desc3(C.Structure):
    _fields_ = [("imax", C.c_int), ("jmax", C.c_int), ("kmax", C.c_int),
                ("xlength", C.c_double), ("ylength", C.c_double), ("zlength", C.c_double),
                ("re", C.c_double), ("gamma", C.c_double), ("tau", C.c_double),
                ("omega", C.c_double), ("eps", C.c_double),
                ("gx", C.c_double), ("gy", C.c_double), ("gz", C.c_double),
                ("itermax", C.c_int),
                ("bcTop", C.c_int), ("bcBottom", C.c_int), ("bcLeft", C.c_int),
                ("bcRight", C.c_int), ("bcFront", C.c_int), ("bcBack", C.c_int),
                ("problem", C.c_int), ("device", C.c_int), ("nranks", C.c_int),
                ("rank", C.c_int), ("comm_id", C.c_void_p)]


class Local3(C.Structure):
    _fields_ = [("n", C.c_int * 3), ("off", C.c_int * 3), ("coords", C.c_int * 3),
                ("dims", C.c_int * 3), ("neighbours", C.c_int * 6)]


# every exported symbol of include/misor.h, with its ctypes signature
SIGNATURES = {
    "misor_last_error": (C.c_char_p, []),
    "misor_version": (C.c_char_p, []),
    "misor_decompose": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                  C.POINTER(Local)]),
    "misor_comm_unique_id": (C.c_int, [C.c_void_p]),
    "misor_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(Desc)]),
    "misor_destroy": (None, [C.c_void_p]),
    "misor_local_info": (C.c_int, [C.c_void_p, C.POINTER(Local)]),
    "misor_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "misor_synchronize": (C.c_int, [C.c_void_p]),
    "misor_upload": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "misor_download": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "misor_fill": (C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    "misor_gather": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "misor_exchange": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "misor_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "misor_comm_ranks": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "misor_poisson_init": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int]),
    "misor_solve_rb": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), _dp]),
    "misor_solve_rb_n": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), _dp]),
    "misor_solve_lex": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), _dp]),
    "misor_mg_default_params": (C.c_int, [C.c_void_p, C.POINTER(MgParams)]),
    "misor_mg_tail": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                C.POINTER(C.c_int)]),
    "misor_mg_levels": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                  C.POINTER(C.c_int), C.c_int]),
    "misor_solve_mg": (C.c_int, [C.c_void_p, C.POINTER(MgParams), C.POINTER(C.c_int), _dp]),
    "misor_solve_mg_dist": (C.c_int, [C.c_void_p, C.POINTER(MgParams), C.c_int,
                                      C.POINTER(C.c_int), _dp]),
    "misor_mg_dist_levels": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "misor_ns_setup": (C.c_int, [C.c_void_p, C.POINTER(NsDesc)]),
    "misor_compute_timestep": (C.c_int, [C.c_void_p, C.c_double, C.c_double, _dp]),
    "misor_set_dt": (C.c_int, [C.c_void_p, C.c_double]),
    "misor_set_boundary_conditions": (C.c_int, [C.c_void_p]),
    "misor_set_special_boundary_condition": (C.c_int, [C.c_void_p]),
    "misor_compute_fg": (C.c_int, [C.c_void_p]),
    "misor_compute_rhs": (C.c_int, [C.c_void_p]),
    "misor_normalize_pressure": (C.c_int, [C.c_void_p]),
    "misor_adapt_uv": (C.c_int, [C.c_void_p]),
    "misor_max_uv": (C.c_int, [C.c_void_p, _dp, _dp]),
    "misor_set_tuning": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "misor_get_tuning": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "misor_enable_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "misor_get_stats": (C.c_int, [C.c_void_p, C.POINTER(StatsDist)]),
    "misor_reset_stats": (C.c_int, [C.c_void_p]),
    "misor_chain_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong,
                                    C.POINTER(C.c_longlong)]),
    "misor_batch_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(BatchDesc)]),
    "misor_batch_destroy": (None, [C.c_void_p]),
    "misor_batch_set_params": (C.c_int, [C.c_void_p, _dp, _dp, C.POINTER(C.c_int)]),
    "misor_batch_upload": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp]),
    "misor_batch_download": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp]),
    "misor_batch_poisson_init": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int]),
    "misor_batch_solve_rb": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), _dp]),
    "misor_batch_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "misor_batch_set_tuning": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "misor_batch_get_tuning": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "misor3_decompose": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                   C.POINTER(C.c_int)]),
    "misor3_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(Desc3)]),
    "misor3_local_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "misor3_gather": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "misor3_destroy": (None, [C.c_void_p]),
    "misor3_upload": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "misor3_download": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "misor3_fill": (C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    "misor3_set_dt": (C.c_int, [C.c_void_p, C.c_double]),
    "misor3_compute_timestep": (C.c_int, [C.c_void_p, _dp]),
    "misor3_max_uvw": (C.c_int, [C.c_void_p, _dp]),
    "misor3_set_boundary_conditions": (C.c_int, [C.c_void_p]),
    "misor3_set_special_boundary_condition": (C.c_int, [C.c_void_p]),
    "misor3_compute_fg": (C.c_int, [C.c_void_p]),
    "misor3_compute_rhs": (C.c_int, [C.c_void_p]),
    "misor3_solve": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), _dp]),
    "misor3_adapt_uvw": (C.c_int, [C.c_void_p]),
    "misor3_normalize_pressure": (C.c_int, [C.c_void_p]),
    "misor3_synchronize": (C.c_int, [C.c_void_p]),
    "misor3_enable_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "misor3_set_tuning": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "misor3_get_tuning": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "misor3_get_solve_time": (C.c_int, [C.c_void_p, _dp, C.POINTER(C.c_longlong)]),
    "misor3_decompose_cart": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int,
                                        C.c_int, C.POINTER(Local3)]),
    "misor3_create_cart": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(Desc3),
                                     C.POINTER(C.c_int)]),
    "misor3_local_info_cart": (C.c_int, [C.c_void_p, C.POINTER(Local3)]),
    "misor3_exchange": (C.c_int, [C.c_void_p, C.c_int]),
    "misor3_mg_default_params": (C.c_int, [C.c_void_p, C.POINTER(MgParams)]),
    "misor3_mg_levels": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                   C.POINTER(C.c_int), C.c_int]),
    "misor3_solve_mg": (C.c_int, [C.c_void_p, C.POINTER(MgParams), C.POINTER(C.c_int), _dp]),
    "misor3_get_mg_info": (C.c_int, [C.c_void_p, C.POINTER(MgInfo3)]),
    "misor3_solve_mg_dist": (C.c_int, [C.c_void_p, C.POINTER(MgParams), C.c_int,
                                       C.POINTER(C.c_int), _dp]),
    "misor3_mg_dist_levels": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.POINTER(C.c_int), C.POINTER(C.c_int)]),
}

_lib = None


class MisorError(RuntimeError):
    pass


# diagnostics that an older library (A/B runs) may lack; the default library must have all
_DIAGNOSTIC = {"misor_chain_trace"}


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIBPATH):
            raise MisorError("libmisor.so not built: run `make -C "
                             "practical-parallel-algorithms-with-mpi_amd` (or __graft_entry__.build())")
        L = C.CDLL(LIBPATH)
        for name, (res, args) in SIGNATURES.items():
            if name in _DIAGNOSTIC and LIBPATH != _DEFAULT_LIBPATH and not hasattr(L, name):
                continue  # an older library loaded for an A/B run (tools/scale_proxy.py --lib)
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise MisorError("libmisor error %d: %s" % (rc, lib().misor_last_error().decode()))


def _ptr(a):
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(_dp)


def decompose(nranks, rank, imax, jmax, dims=(0, 0)):
    loc = Local()
    d = (C.c_int * 2)(*dims)
    _check(lib().misor_decompose(nranks, rank, imax, jmax, d, C.byref(loc)))
    return loc


def mg_levels(imax, jmax, coarse_cells=64):
    """[(imax, jmax), ...] of the multigrid levels of an imax x jmax grid, level 0
    first (misor_mg_levels; host-only)"""
    n = C.c_int(0)
    _check(lib().misor_mg_levels(imax, jmax, coarse_cells, C.byref(n), None, 0))
    shapes = (C.c_int * (2 * n.value))()
    _check(lib().misor_mg_levels(imax, jmax, coarse_cells, C.byref(n), shapes, n.value))
    return [(shapes[2 * k], shapes[2 * k + 1]) for k in range(n.value)]


def mg_tail(imax, jmax, coarse_cells=64):
    """(first, count) of the tail of mg_levels(imax, jmax, coarse_cells): its trailing
    levels that each fit the LDS of one workgroup; count 0 (first = the number of
    levels): none does (misor_mg_tail; host-only)"""
    first, count = C.c_int(0), C.c_int(0)
    _check(lib().misor_mg_tail(imax, jmax, coarse_cells, C.byref(first), C.byref(count)))
    return first.value, count.value


def mg_dist_levels(nranks, imax, jmax, coarse_cells=64, gather_cells=-1, dims=(0, 0)):
    """(nlevels, ndist): the levels of an imax x jmax grid and how many of them
    misor_solve_mg_dist keeps distributed over nranks (misor_mg_dist_levels;
    host-only)"""
    n, nd = C.c_int(0), C.c_int(0)
    d = (C.c_int * 2)(*dims)
    _check(lib().misor_mg_dist_levels(nranks, d, imax, jmax, coarse_cells, gather_cells,
                                      C.byref(n), C.byref(nd)))
    return n.value, nd.value


def mg3_levels(imax, jmax, kmax, coarse_cells=512):
    """[(imax, jmax, kmax), ...] of the 3D multigrid levels, level 0 first
    (misor3_mg_levels; host-only)"""
    n = C.c_int(0)
    _check(lib().misor3_mg_levels(imax, jmax, kmax, coarse_cells, C.byref(n), None, 0))
    shapes = (C.c_int * (3 * n.value))()
    _check(lib().misor3_mg_levels(imax, jmax, kmax, coarse_cells, C.byref(n), shapes, n.value))
    return [tuple(shapes[3 * k:3 * k + 3]) for k in range(n.value)]


def mg3_dist_levels(nranks, imax, jmax, kmax, coarse_cells=512, gather_cells=-1):
    """(nlevels, ndist): the levels of an imax x jmax x kmax grid and how many of
    them misor3_solve_mg_dist keeps distributed over nranks slabs
    (misor3_mg_dist_levels; host-only)"""
    n, nd = C.c_int(0), C.c_int(0)
    _check(lib().misor3_mg_dist_levels(nranks, imax, jmax, kmax, coarse_cells, gather_cells,
                                       C.byref(n), C.byref(nd)))
    return n.value, nd.value


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(lib().misor_comm_unique_id(buf))
    return buf.raw


class Grid:
    """One rank's device-resident grid (the Solver struct's arrays in HBM)."""

    def __init__(self, imax, jmax, dx, dy, omega, eps, itermax, variant=SOLVE_RB, device=-1,
                 nranks=1, rank=0, dims=(0, 0), comm_id: bytes | None = None):
        d = Desc()
        d.imax, d.jmax, d.dx, d.dy = imax, jmax, dx, dy
        d.omega, d.eps, d.itermax, d.variant = omega, eps, itermax, variant
        d.device, d.nranks, d.rank = device, nranks, rank
        d.dims[0], d.dims[1] = dims
        self._id = C.create_string_buffer(comm_id, COMM_ID_BYTES) if comm_id else None
        d.comm_id = C.cast(self._id, C.c_void_p) if self._id is not None else None
        self.h = C.c_void_p()
        _check(lib().misor_create(C.byref(self.h), C.byref(d)))
        self.desc = d
        self.loc = Local()
        _check(lib().misor_local_info(self.h, C.byref(self.loc)))
        self.shape = (self.loc.nj + 2, self.loc.ni + 2)
        self.imax, self.jmax, self.rank, self.nranks = imax, jmax, rank, nranks

    def close(self):
        if self.h:
            lib().misor_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, field, arr):
        a = np.ascontiguousarray(arr, dtype=np.float64)
        assert a.shape == self.shape, (a.shape, self.shape)
        _check(lib().misor_upload(self.h, field, _ptr(a)))

    def download(self, field):
        a = np.empty(self.shape)
        _check(lib().misor_download(self.h, field, _ptr(a)))
        return a

    def gather(self, field):
        """collectResult: the global (jmax+2, imax+2) field on rank 0, None elsewhere
        (collective: every rank of the grid must call it)"""
        if self.rank == 0:
            out = np.empty((self.jmax + 2, self.imax + 2))
            _check(lib().misor_gather(self.h, field, _ptr(out)))
            return out
        _check(lib().misor_gather(self.h, field, C.cast(None, _dp)))
        return None

    def exchange(self, field, depth=1):
        """exchange (skeleton/src/solver.c:137-165): the depth-deep halo of
        `field` from the 8 neighbours (collective)"""
        _check(lib().misor_exchange(self.h, field, depth))

    def fill(self, field, value):
        _check(lib().misor_fill(self.h, field, value))

    def poisson_init(self, xlength, ylength, problem=2):
        _check(lib().misor_poisson_init(self.h, xlength, ylength, problem))

    def solve_rb(self, itermax=None):
        it = C.c_int(0)
        res = C.c_double(0.0)
        if itermax is None:
            _check(lib().misor_solve_rb(self.h, C.byref(it), C.byref(res)))
        else:
            _check(lib().misor_solve_rb_n(self.h, itermax, C.byref(it), C.byref(res)))
        return it.value, res.value

    def solve_lex(self, xorder=0):
        """lexicographic SOR (the reference's `solve`); xorder 0 = assignment-4,
        1 = assignment-5 sequential"""
        it, res = C.c_int(0), C.c_double(0.0)
        _check(lib().misor_solve_lex(self.h, xorder, C.byref(it), C.byref(res)))
        return it.value, res.value

    def mg_default_params(self):
        q = MgParams()
        _check(lib().misor_mg_default_params(self.h, C.byref(q)))
        return q

    def solve_mg(self, **params):
        """multigrid V-cycles (misor_solve_mg): (cycles, res).  Keywords are
        the fields of misor_mg_params (nu1, nu2, omega_smooth, coarse_cells,
        omega_coarse, eps_coarse, itermax_coarse, maxcycles); those not given
        keep their defaults"""
        q = self.mg_default_params()
        names = [f[0] for f in MgParams._fields_]
        for k, v in params.items():
            if k not in names:
                raise TypeError("solve_mg: unknown parameter %r (one of %s)" % (k, names))
            setattr(q, k, v)
        n, res = C.c_int(0), C.c_double(0.0)
        _check(lib().misor_solve_mg(self.h, C.byref(q), C.byref(n), C.byref(res)))
        return n.value, res.value

    def solve_mg_dist(self, gather_cells=-1, **params):
        """multigrid V-cycles on a decomposed grid (misor_solve_mg_dist; collective):
        (cycles, res).  gather_cells: blocks of at most this many cells are
        gathered (-1: the default); the other keywords as solve_mg's"""
        q = self.mg_default_params()
        names = [f[0] for f in MgParams._fields_]
        for k, v in params.items():
            if k not in names:
                raise TypeError("solve_mg_dist: unknown parameter %r (one of %s)" % (k, names))
            setattr(q, k, v)
        n, res = C.c_int(0), C.c_double(0.0)
        _check(lib().misor_solve_mg_dist(self.h, C.byref(q), gather_cells, C.byref(n),
                                         C.byref(res)))
        return n.value, res.value

    def synchronize(self):
        _check(lib().misor_synchronize(self.h))

    def comm_ranks(self):
        """ranks of the grid's communicator as the transport counts them
        (ncclCommCount for RCCL)"""
        n = C.c_int(0)
        _check(lib().misor_comm_ranks(self.h, C.byref(n)))
        return n.value

    def set_stream(self, stream_ptr):
        _check(lib().misor_set_stream(self.h, C.c_void_p(stream_ptr)))

    # ---- NS
    def ns_setup(self, prm: dict):
        n = NsDesc()
        n.xlength, n.ylength = prm["xlength"], prm["ylength"]
        n.re, n.gx, n.gy = prm["re"], prm["gx"], prm["gy"]
        n.gamma, n.tau = prm["gamma"], prm["tau"]
        n.bcLeft, n.bcRight = int(prm["bcLeft"]), int(prm["bcRight"])
        n.bcBottom, n.bcTop = int(prm["bcBottom"]), int(prm["bcTop"])
        n.problem = {"dcavity": PROBLEM_DCAVITY, "canal": PROBLEM_CANAL}.get(
            prm.get("name") or "", PROBLEM_NONE)
        _check(lib().misor_ns_setup(self.h, C.byref(n)))

    def compute_timestep(self, dt_bound, tau):
        dt = C.c_double(0.0)
        _check(lib().misor_compute_timestep(self.h, dt_bound, tau, C.byref(dt)))
        return dt.value

    def set_dt(self, dt):
        _check(lib().misor_set_dt(self.h, dt))

    def max_uv(self):
        a, b = C.c_double(0.0), C.c_double(0.0)
        _check(lib().misor_max_uv(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def call(self, name):
        _check(getattr(lib(), "misor_" + name)(self.h))

    # ---- tuning (launch geometry only; results are bit-identical)
    def set_tuning(self, key, value):
        _check(lib().misor_set_tuning(self.h, key, value))

    def get_tuning(self, key):
        v = C.c_int(0)
        _check(lib().misor_get_tuning(self.h, key, C.byref(v)))
        return v.value

    # ---- stats
    def enable_timing(self, on=True):
        _check(lib().misor_enable_timing(self.h, 1 if on else 0))

    def stats(self):
        s = StatsDist()
        _check(lib().misor_get_stats(self.h, C.byref(s)))
        return {"sweeps": s.sweeps, "launches": s.launches, "sweep_ms": s.sweep_ms,
                "timed_sweeps": s.timed_sweeps, "timed_passes": s.timed_passes,
                "iters_per_pass": s.iters_per_pass, "tb_variant": s.tb_variant,
                "halo_ms": s.halo_ms, "halos": s.halos,
                "allreduce_ms": s.allreduce_ms, "allreduces": s.allreduces,
                "chained": s.chained, "ns_ms": list(s.ns_ms), "ns_calls": list(s.ns_calls),
                "lite_misses": s.lite_misses, "mg_cycles": s.mg_cycles,
                "mg_levels": s.mg_levels, "mg_transfer_ms": list(s.mg_transfer_ms),
                "mg_transfers": s.mg_transfers, "mg_tail_levels": s.mg_tail_levels,
                "mg_tail_launches": s.mg_tail_launches,
                "mg_tail_fallbacks": s.mg_tail_fallbacks, "mg_tail_ms": s.mg_tail_ms,
                "mg_dist_levels": s.mg_dist_levels}

    def reset_stats(self):
        _check(lib().misor_reset_stats(self.h))

    def chain_trace(self):
        """per-block timeline of the last chained pass (MISOR_CHAIN_TRACE=1 at
        configure time): array (blocks, 3) of start, end (100 MHz clock) and
        workgroup | 1 << 32 for a run's first block | 1 << 33 for a block run by
        the edge kernel (both kernels number their workgroups from 0); row
        L = by * nbx + bx; None if not traced"""
        import numpy as np
        n = C.c_longlong(0)
        _check(lib().misor_chain_trace(self.h, None, 0, C.byref(n)))
        if n.value == 0:
            return None
        out = np.zeros(n.value, dtype=np.uint64)
        _check(lib().misor_chain_trace(self.h, out.ctypes.data, n.value, C.byref(n)))
        return out.reshape(-1, 3)


class Batch:
    """nbatch independent Poisson problems of one shape, solved in one launch
    (misor_batch_*): per-member omega, eps, itermax, p and rhs.  Host arrays
    are (nbatch, jmax+2, imax+2), or (jmax+2, imax+2) for one member."""

    def __init__(self, imax, jmax, dx, dy, nbatch, variant=SOLVE_RB, device=-1):
        d = BatchDesc()
        d.imax, d.jmax, d.dx, d.dy = imax, jmax, dx, dy
        d.nbatch, d.variant, d.device = nbatch, variant, device
        self.h = C.c_void_p()
        _check(lib().misor_batch_create(C.byref(self.h), C.byref(d)))
        self.desc = d
        self.imax, self.jmax, self.nbatch = imax, jmax, nbatch
        self.shape = (jmax + 2, imax + 2)

    def close(self):
        if self.h:
            lib().misor_batch_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _per_member(self, v, dtype):
        """None, a scalar for every member, or a length-nbatch sequence"""
        if v is None:
            return None
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (self.nbatch,)))
        return a

    def set_params(self, omega=None, eps=None, itermax=None):
        om = self._per_member(omega, np.float64)
        ep = self._per_member(eps, np.float64)
        im = self._per_member(itermax, np.intc)
        _check(lib().misor_batch_set_params(
            self.h, None if om is None else _ptr(om), None if ep is None else _ptr(ep),
            None if im is None else im.ctypes.data_as(C.POINTER(C.c_int))))

    def upload(self, field, arr, member=None):
        a = np.ascontiguousarray(arr, dtype=np.float64)
        want = self.shape if member is not None else (self.nbatch,) + self.shape
        assert a.shape == want, (a.shape, want)
        _check(lib().misor_batch_upload(self.h, field, -1 if member is None else member, _ptr(a)))

    def download(self, field, member=None):
        a = np.empty(self.shape if member is not None else (self.nbatch,) + self.shape)
        _check(lib().misor_batch_download(self.h, field, -1 if member is None else member,
                                          _ptr(a)))
        return a

    def poisson_init(self, xlength, ylength, problem=2):
        _check(lib().misor_batch_poisson_init(self.h, xlength, ylength, problem))

    def solve_rb(self):
        """(iters, res): int and float64 arrays of nbatch"""
        it = np.zeros(self.nbatch, dtype=np.intc)
        res = np.zeros(self.nbatch)
        _check(lib().misor_batch_solve_rb(self.h, it.ctypes.data_as(C.POINTER(C.c_int)),
                                          _ptr(res)))
        return it, res

    def set_stream(self, stream_ptr):
        _check(lib().misor_batch_set_stream(self.h, C.c_void_p(stream_ptr)))

    def set_tuning(self, key, value):
        _check(lib().misor_batch_set_tuning(self.h, key, value))

    def get_tuning(self, key):
        v = C.c_int(0)
        _check(lib().misor_batch_get_tuning(self.h, key, C.byref(v)))
        return v.value


_PROBLEMS = {"dcavity": PROBLEM_DCAVITY, "canal": PROBLEM_CANAL}


def decompose3(nranks, rank, kmax):
    """(kloc, koff) of rank's slab"""
    a, b = C.c_int(0), C.c_int(0)
    _check(lib().misor3_decompose(nranks, rank, kmax, C.byref(a), C.byref(b)))
    return a.value, b.value


def decompose3_cart(nranks, rank, imax, jmax, kmax, dims=(0, 0, 0)):
    """the Local3 block of `rank` on the process grid dims = (x, y, z); 0: automatic"""
    loc = Local3()
    d = (C.c_int * 3)(*dims)
    _check(lib().misor3_decompose_cart(nranks, rank, d, imax, jmax, kmax, C.byref(loc)))
    return loc


class Grid3:
    """The 3D solver (assignment-6/src/solver.c): fields of shape
    (kloc+2, jmax+2, imax+2), A(i,j,k) = a[k, j, i] (solver.c:19-34); kloc =
    kmax on one GPU, the rank's slab when decomposed (nranks > 1).  With dims =
    (x, y, z) the box is split over that Cartesian process grid instead (0
    entries: automatic): fields of shape (nk+2, nj+2, ni+2) with .n = (ni, nj,
    nk), and .off, .coords, .dims, .neighbours as misor3_local."""

    def __init__(self, prm: dict, device=-1, nranks=1, rank=0, comm_id: bytes | None = None,
                 dims=None):
        d = Desc3()
        d.imax, d.jmax, d.kmax = int(prm["imax"]), int(prm["jmax"]), int(prm["kmax"])
        d.xlength, d.ylength, d.zlength = prm["xlength"], prm["ylength"], prm["zlength"]
        d.re, d.gamma, d.tau = prm["re"], prm["gamma"], prm["tau"]
        d.omega, d.eps, d.itermax = prm["omg"], prm["eps"], int(prm["itermax"])
        d.gx, d.gy, d.gz = prm["gx"], prm["gy"], prm["gz"]
        for k in ("bcTop", "bcBottom", "bcLeft", "bcRight", "bcFront", "bcBack"):
            setattr(d, k, int(prm[k]))
        d.problem = _PROBLEMS.get(prm.get("name") or "", PROBLEM_NONE)
        d.device = device
        d.nranks, d.rank = nranks, rank
        self._id = C.create_string_buffer(comm_id, COMM_ID_BYTES) if comm_id else None
        d.comm_id = C.cast(self._id, C.c_void_p) if self._id is not None else None
        self.h = C.c_void_p()
        if dims is None:
            _check(lib().misor3_create(C.byref(self.h), C.byref(d)))
        else:
            _check(lib().misor3_create_cart(C.byref(self.h), C.byref(d), (C.c_int * 3)(*dims)))
        self.desc = d
        a, b = C.c_int(0), C.c_int(0)
        _check(lib().misor3_local_info(self.h, C.byref(a), C.byref(b)))
        self.kloc, self.koff = a.value, b.value
        self.rank, self.nranks = rank, nranks
        loc = Local3()
        _check(lib().misor3_local_info_cart(self.h, C.byref(loc)))
        self.n, self.off = tuple(loc.n), tuple(loc.off)
        self.coords, self.dims = tuple(loc.coords), tuple(loc.dims)
        self.neighbours = tuple(loc.neighbours)
        self.shape = (self.n[2] + 2, self.n[1] + 2, self.n[0] + 2)
        self.global_shape = (d.kmax + 2, d.jmax + 2, d.imax + 2)

    def close(self):
        if self.h:
            lib().misor3_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, field, arr):
        a = np.ascontiguousarray(arr, dtype=np.float64)
        assert a.shape == self.shape, (a.shape, self.shape)
        _check(lib().misor3_upload(self.h, field, _ptr(a)))

    def download(self, field):
        a = np.empty(self.shape)
        _check(lib().misor3_download(self.h, field, _ptr(a)))
        return a

    def fill(self, field, value):
        _check(lib().misor3_fill(self.h, field, value))

    def gather(self, field):
        """the global field on rank 0, None elsewhere (collective)"""
        if self.rank == 0:
            out = np.empty(self.global_shape)
            _check(lib().misor3_gather(self.h, field, _ptr(out)))
            return out
        _check(lib().misor3_gather(self.h, field, C.cast(None, _dp)))
        return None

    def exchange(self, field):
        """the 1-deep halo of `field`, edges and corners included (collective;
        Cartesian grids)"""
        _check(lib().misor3_exchange(self.h, field))

    def set_dt(self, dt):
        _check(lib().misor3_set_dt(self.h, dt))

    def compute_timestep(self):
        dt = C.c_double(0.0)
        _check(lib().misor3_compute_timestep(self.h, C.byref(dt)))
        return dt.value

    def max_uvw(self):
        m = (C.c_double * 3)()
        _check(lib().misor3_max_uvw(self.h, C.cast(m, _dp)))
        return tuple(m)

    def solve(self):
        it, res = C.c_int(0), C.c_double(0.0)
        _check(lib().misor3_solve(self.h, C.byref(it), C.byref(res)))
        return it.value, res.value

    def enable_timing(self, on=True):
        _check(lib().misor3_enable_timing(self.h, 1 if on else 0))

    def set_tuning(self, key, value):
        _check(lib().misor3_set_tuning(self.h, key, value))

    def get_tuning(self, key):
        v = C.c_int(0)
        _check(lib().misor3_get_tuning(self.h, key, C.byref(v)))
        return v.value

    def mg_default_params(self):
        """nu1 = nu2 = 2, omega_smooth 1.0, coarse_cells 512, omega_coarse 1.7,
        eps_coarse 0.1 eps, itermax_coarse 1000, maxcycles 100"""
        q = MgParams()
        _check(lib().misor3_mg_default_params(self.h, C.byref(q)))
        return q

    def solve_mg(self, **params):
        """multigrid V-cycles (misor3_solve_mg): (cycles, res).  Keywords are
        the fields of misor_mg_params; those not given keep their 3D defaults"""
        q = self.mg_default_params()
        names = [f[0] for f in MgParams._fields_]
        for k, v in params.items():
            if k not in names:
                raise TypeError("solve_mg: unknown parameter %r (one of %s)" % (k, names))
            setattr(q, k, v)
        n, res = C.c_int(0), C.c_double(0.0)
        _check(lib().misor3_solve_mg(self.h, C.byref(q), C.byref(n), C.byref(res)))
        return n.value, res.value

    def solve_mg_dist(self, gather_cells=-1, **params):
        """multigrid V-cycles on slabs (misor3_solve_mg_dist; collective): (cycles,
        res).  gather_cells: halved slabs of at most that many cells are gathered
        (-1: the default); the other keywords as solve_mg's"""
        q = self.mg_default_params()
        names = [f[0] for f in MgParams._fields_]
        for k, v in params.items():
            if k not in names:
                raise TypeError("solve_mg_dist: unknown parameter %r (one of %s)" % (k, names))
            setattr(q, k, v)
        n, res = C.c_int(0), C.c_double(0.0)
        _check(lib().misor3_solve_mg_dist(self.h, C.byref(q), gather_cells, C.byref(n),
                                          C.byref(res)))
        return n.value, res.value

    def mg_info(self):
        """the last solve_mg / solve_mg_dist: cycles, levels; with timing on the
        device ms of level 0's two transfer kernels and the launches they cover;
        ["dist_levels"]: the levels the last solve kept distributed.  Where that is 0
        (solve_mg, one rank) it is no entry of the dict -- `in`, .get(), .items() and
        dict() do not see it -- and only indexing gives the 0"""
        s = MgInfo3()
        _check(lib().misor3_get_mg_info(self.h, C.byref(s)))
        out = _MgInfo3Dict(cycles=s.cycles, levels=s.levels, transfer_ms=list(s.transfer_ms),
                           transfers=s.transfers)
        if s.dist_levels:
            out["dist_levels"] = s.dist_levels
        return out

    def solve_time(self):
        """(device ms, iterations) of the solves timed since enable_timing"""
        ms, it = C.c_double(0.0), C.c_longlong(0)
        _check(lib().misor3_get_solve_time(self.h, C.byref(ms), C.byref(it)))
        return ms.value, it.value

    def call(self, name):
        """set_boundary_conditions, set_special_boundary_condition, compute_fg,
        compute_rhs, adapt_uvw, normalize_pressure, synchronize"""
        _check(getattr(lib(), "misor3_" + name)(self.h))
