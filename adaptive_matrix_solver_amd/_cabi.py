"""ctypes binding of libmaus_hip.so (include/maus_hip.h).

The product path has no CPU fallback: if the HIP library cannot be loaded, or a
device context cannot be created, this module raises -- it never routes the
candidate step through NumPy/SciPy."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .band import DIRECT_METHOD

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmaus_hip.so")

# every symbol include/maus_hip.h declares (tests/test_cabi_symbols.py checks the list against the header)
SYMBOLS = [
    "maus_ctx_create", "maus_ctx_destroy", "maus_last_error", "maus_device_info", "maus_abi_version", "maus_lu_max_n",
    "maus_set_matrix", "maus_set_matrix_csr", "maus_matrix_is_sparse", "maus_set_rhs", "maus_pop_reserve", "maus_pop_capacity", "maus_pop_put", "maus_pop_get", "maus_pop_copy", "maus_pop_device_ptr", "maus_hist_append", "maus_hist_get", "maus_hist_clear", "maus_hist_generation",
    "maus_matvec_rayleigh", "maus_shifted_lu_solve", "maus_lu_reserve", "maus_lu_workspace_allocs", "maus_set_shared_device", "maus_lu_mw_aborts", "maus_relax_normalise", "maus_residual",
    "maus_svd_power_step", "maus_svd_power_propose", "maus_svd_commit", "maus_set_eigvecs", "maus_herm_match", "maus_herm_tridiag", "maus_herm_set_chunk", "maus_herm_chunk_plan", "maus_herm_release", "maus_herm_tridiag_eig", "maus_herm_tridiag_eigvals", "maus_herm_backtransform", "maus_get_eigvecs", "maus_gmres", "maus_gmres_pert", "maus_jacobi_check",
    "maus_profile_union_ms", "maus_gram", "maus_zgemm_host", "maus_lu_solve_host", "maus_timer_start", "maus_timer_stop",
    "maus_profile_enable", "maus_profile_read", "maus_sync", "maus_mt19937_jump",
    "maus_lanczos_begin", "maus_lanczos_inject", "maus_lanczos_extend", "maus_lanczos_restart", "maus_lanczos_finish", "maus_herm_match_rows", "maus_get_ritz_rows", "maus_lanczos_get_basis",
    "maus_sparse_max_n", "maus_band_prepare", "maus_band_reserve", "maus_band_solve", "maus_band_lu_host", "maus_band_workspace_allocs",
    "maus_band_set_method", "maus_band_get_method", "maus_band_kernel_for", "maus_band_outer_nb", "maus_band_plan",
    "maus_band_set_split", "maus_band_get_split", "maus_band_split_plan",
    "maus_band_set_real", "maus_band_get_real", "maus_band_real_plan", "maus_band_real_kinds",
    "maus_gmres_set_method", "maus_gmres_get_method", "maus_gmres_kernel_for",
    "maus_real_set_method", "maus_real_get_method", "maus_real_plan", "maus_real_spmm", "maus_real_values_flagged",
    "maus_few_rows_set_method", "maus_few_rows_get_method", "maus_few_rows_kernel_for", "maus_few_rows_plan", "maus_few_rows_workspace_allocs",
    "maus_zgemm_plan",
    "maus_pop_draw", "maus_pop_draw_plan", "maus_pop_draw_min_len",
    "maus_spmm_set_method", "maus_spmm_get_method", "maus_spmm_kernel_for", "maus_spmm_plan", "maus_spmm_sell_info",
    "maus_device_count", "maus_comm_unique_id", "maus_comm_init", "maus_comm_destroy", "maus_comm_info",
    "maus_comm_allgather_records", "maus_comm_allgather_rows", "maus_comm_bcast", "maus_comm_bcast_eigvecs", "maus_comm_set_matrix", "maus_comm_stats",
]

COMM_ID_BYTES = 128

POP_X, POP_U, POP_W, POP_Y = 0, 1, 2, 3
KIND_EIG, KIND_LINEAR, KIND_SVD = 1, 2, 3
PERT_NONE, PERT_UNIFORM, PERT_MT19937 = 0, 1, 2
KC_NAMES = ["zgemm", "lu_panel", "trsm", "laswp", "build_h", "backsolve", "vector",
            "zgemm_k128", "zgemm_k64", "zgemm_k32", "zgemm_k16", "spmm", "band", "lanczos", "band_blocked", "band_tiled", "band_wide", "gmres_wide"]
KC_BAND_SPLIT = len(KC_NAMES)      # band solves by the split method (maus_band_set_split): read as "band_split", behind the named classes
BAND_COLUMN, BAND_BLOCKED, BAND_TILED, BAND_WIDE, BAND_NARROW = (      # maus_band_set_method: 0, 1, 2, 4, 8 (no 3, 5, 6, 7)
    DIRECT_METHOD[m] for m in ("band", "blocked", "tiled", "wide", "narrow"))
GMRES_DEFAULT, GMRES_WIDE = 0, 1                     # maus_gmres_set_method
REAL_OFF, REAL_ON = 0, 1                             # maus_real_set_method
# maus_real_plan: why a call runs complex (the first condition of the rule that fails), or REAL_OK
REAL_OK, REAL_METHOD_OFF, REAL_NOT_CSR, REAL_MATRIX_COMPLEX, REAL_RHS_ROWS, REAL_RHS_COMPLEX, REAL_SHIFT_COMPLEX = range(7)
KC_GMRES_REAL, KC_SPMM_REAL = 19, 20                 # the real path's post step and products: read as "gmres_real" / "spmm_real", behind the named classes
BAND_REAL_OFF, BAND_REAL_ON = 0, 1                   # maus_band_set_real
# maus_band_real_plan: why a band solve runs complex (the first condition of the rule that fails), or BAND_REAL_OK
(BAND_REAL_OK, BAND_REAL_MODE_OFF, BAND_REAL_NOT_CSR, BAND_REAL_MATRIX_COMPLEX, BAND_REAL_RHS_ROWS, BAND_REAL_RHS_COMPLEX,
 BAND_REAL_SHIFT_COMPLEX, BAND_REAL_NO_KERNELS) = range(8)
KC_BAND_REAL = 21                                    # band solves of the real path: read as "band_real", behind the named classes
FEW_ROWS_DEFAULT, FEW_ROWS_SPLITK = 0, 1             # maus_few_rows_set_method
ZGEMM_ROWS, ZGEMM_LU = 0, 1                          # maus_zgemm_plan: the form ...
LU_TILE_DEFAULT, LU_TILE_64X64, LU_TILE_128X64 = 0, 1, 2   # ... what MAUS_LU_TILE selects ...
ZGEMM_4M, ZGEMM_3M, ZGEMM_3M_DMA = 0, 1, 2           # ... and the kernel family it returns
SPMM_SCHEDULES = {0: None, 1: "rows", 2: "wave"}     # maus_matrix_is_sparse: dense / lane per row / wave per row
DRAW_RAW, DRAW_UNIT, DRAW_NORM = 0, 1, 2             # maus_pop_draw: kinds
SPMM_CSR, SPMM_SELL = 0, 1                           # maus_spmm_set_method
SPMM_KERNEL_NONE, SPMM_KERNEL_ROWS, SPMM_KERNEL_WAVE, SPMM_KERNEL_SELL = 0, 1, 2, 3   # maus_spmm_kernel_for / maus_spmm_plan



class MtDesc(C.Structure):
    """maus_mt_desc (include/maus_hip.h)."""
    _fields_ = [("key", C.c_uint32 * 624), ("pos", C.c_int32), ("reserved", C.c_int32),
                ("words_per_candidate", C.c_uint64), ("lead_words", C.c_uint64), ("ordinals", C.POINTER(C.c_int32))]


_lib = None


class MausHipError(RuntimeError):
    pass


def load_library():
    """Load libmaus_hip.so (built in-tree by __graft_entry__.build()).  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MausHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the candidate step.")
    lib = C.CDLL(LIB_PATH)
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
    i32p = C.POINTER(C.c_int32)
    sig = {
        "maus_ctx_create": ([C.c_int, C.POINTER(vp)], C.c_int),
        "maus_ctx_destroy": ([vp], C.c_int),
        "maus_last_error": ([vp], C.c_char_p),
        "maus_device_info": ([vp, C.c_char_p, C.c_int, ip, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)], C.c_int),
        "maus_abi_version": ([], C.c_int),
        "maus_lu_max_n": ([], C.c_int),
        "maus_set_matrix": ([vp, vp, C.c_int, C.c_int], C.c_int),
        "maus_set_matrix_csr": ([vp, C.c_int, C.c_int, C.c_int64, vp, vp, vp], C.c_int),
        "maus_matrix_is_sparse": ([vp], C.c_int),
        "maus_set_rhs": ([vp, vp, C.c_int], C.c_int),
        "maus_pop_reserve": ([vp, C.c_int], C.c_int),
        "maus_pop_capacity": ([vp], C.c_int),
        "maus_pop_put": ([vp, C.c_int, vp, C.c_int, vp, C.c_int], C.c_int),
        "maus_pop_get": ([vp, C.c_int, vp, C.c_int, vp, C.c_int], C.c_int),
        "maus_pop_copy": ([vp, C.c_int, C.c_int, vp, C.c_int], C.c_int),
        "maus_pop_device_ptr": ([vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_long), ip], C.c_int),
        "maus_hist_append": ([vp, C.c_int, vp, C.c_int, C.c_int, C.POINTER(C.c_int64)], C.c_int),
        "maus_hist_get": ([vp, vp, C.c_int, C.c_int, vp], C.c_int),
        "maus_hist_clear": ([vp], C.c_int),
        "maus_hist_generation": ([vp], C.c_int64),
        "maus_matvec_rayleigh": ([vp, vp, C.c_int, vp, vp], C.c_int),
        "maus_shifted_lu_solve": ([vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp], C.c_int),
        "maus_lu_reserve": ([vp, C.c_int, C.c_int, ip], C.c_int),
        "maus_lu_workspace_allocs": ([vp], C.c_int),
        "maus_set_shared_device": ([vp, C.c_int], C.c_int),
        "maus_lu_mw_aborts": ([vp], C.c_int),
        "maus_relax_normalise": ([vp, vp, C.c_int, vp, C.c_int, vp], C.c_int),
        "maus_residual": ([vp, C.c_int, vp, C.c_int, vp, vp, vp], C.c_int),
        "maus_svd_power_step": ([vp, vp, C.c_int, vp], C.c_int),
        "maus_svd_power_propose": ([vp, vp, C.c_int, vp], C.c_int),
        "maus_svd_commit": ([vp, vp, C.c_int], C.c_int),
        "maus_set_eigvecs": ([vp, vp, C.c_int], C.c_int),
        "maus_herm_match": ([vp, vp, C.c_int, vp, vp], C.c_int),
        "maus_herm_tridiag": ([vp, vp, vp], C.c_int),
        "maus_herm_release": ([vp], C.c_int),
        "maus_herm_set_chunk": ([vp, C.c_int], C.c_int),
        "maus_herm_chunk_plan": ([C.c_int, C.c_int, C.c_int, ip, ip, ip], C.c_int),
        "maus_herm_backtransform": ([vp, vp, C.c_int], C.c_int),
        "maus_herm_tridiag_eig": ([vp, vp, vp, C.c_int, vp, vp], C.c_int),
        "maus_herm_tridiag_eigvals": ([vp, vp, vp, C.c_int, vp], C.c_int),
        "maus_get_eigvecs": ([vp, vp, C.c_int], C.c_int),
        "maus_gmres": ([vp, vp, C.c_int, vp, vp, C.c_int, vp, C.c_double, C.c_int, C.c_int, vp, vp, vp], C.c_int),
        "maus_gmres_pert": ([vp, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, C.c_double, C.c_int, C.c_int, vp, vp, vp, vp], C.c_int),
        "maus_jacobi_check": ([vp, C.c_int, vp, vp, vp], C.c_int),
        "maus_profile_union_ms": ([vp, C.c_int, C.POINTER(C.c_double)], C.c_int),
        "maus_gram": ([vp, C.c_int, vp, C.c_int, C.c_int, vp], C.c_int),
        "maus_zgemm_host": ([vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int], C.c_int),
        "maus_lu_solve_host": ([vp, C.c_int, C.c_int, vp, vp, vp, vp, vp], C.c_int),
        "maus_timer_start": ([vp], C.c_int),
        "maus_timer_stop": ([vp, C.POINTER(C.c_float)], C.c_int),
        "maus_profile_enable": ([vp, C.c_int], C.c_int),
        "maus_profile_read": ([vp, C.c_int, ip, dp, dp, dp], C.c_int),
        "maus_sync": ([vp], C.c_int),
        "maus_mt19937_jump": ([vp, i32p, C.c_uint64], C.c_int),
        "maus_lanczos_begin": ([vp, vp, C.c_int], C.c_int),
        "maus_lanczos_inject": ([vp, C.c_int, vp], C.c_int),
        "maus_lanczos_extend": ([vp, C.c_int, C.c_int, C.c_double, vp, vp], C.c_int),
        "maus_lanczos_restart": ([vp, vp, C.c_int, C.c_int], C.c_int),
        "maus_lanczos_finish": ([vp, vp, C.c_int, C.c_int], C.c_int),
        "maus_herm_match_rows": ([vp, vp, C.c_int, vp, vp], C.c_int),
        "maus_get_ritz_rows": ([vp, vp, C.c_int, C.c_int], C.c_int),
        "maus_lanczos_get_basis": ([vp, C.c_int, C.c_int, vp], C.c_int),
        "maus_sparse_max_n": ([], C.c_int),
        "maus_band_prepare": ([vp, vp, C.c_int, ip, ip], C.c_int),
        "maus_band_reserve": ([vp, C.c_int, ip], C.c_int),
        "maus_band_solve": ([vp, vp, C.c_int, vp, vp, C.c_int, vp], C.c_int),
        "maus_band_lu_host": ([vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp], C.c_int),
        "maus_band_workspace_allocs": ([vp], C.c_int),
        "maus_band_set_method": ([vp, C.c_int], C.c_int),
        "maus_band_get_method": ([vp], C.c_int),
        "maus_band_kernel_for": ([vp, C.c_int, C.c_int, C.c_int, ip], C.c_int),
        "maus_gmres_set_method": ([vp, C.c_int], C.c_int),
        "maus_gmres_get_method": ([vp], C.c_int),
        "maus_gmres_kernel_for": ([vp, C.c_int, C.c_int], C.c_int),
        "maus_real_set_method": ([vp, C.c_int], C.c_int),
        "maus_real_get_method": ([vp], C.c_int),
        "maus_real_plan": ([vp, C.c_int, C.c_int, vp, vp], C.c_int),
        "maus_real_spmm": ([vp, vp, C.c_int], C.c_int),
        "maus_real_values_flagged": ([vp, C.c_int64], C.c_int),
        "maus_few_rows_set_method": ([vp, C.c_int, C.c_int], C.c_int),
        "maus_few_rows_get_method": ([vp], C.c_int),
        "maus_few_rows_kernel_for": ([vp] + [C.c_int] * 6 + [C.POINTER(C.c_int)], C.c_int),
        "maus_few_rows_plan": ([C.c_int] * 8 + [C.POINTER(C.c_int)], C.c_int),
        "maus_few_rows_workspace_allocs": ([vp], C.c_int),
        "maus_zgemm_plan": ([C.c_int] * 9 + [ip, ip], C.c_int),
        "maus_pop_draw": ([vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp], C.c_int),
        "maus_pop_draw_plan": ([C.c_int, C.c_int, vp, C.c_int, C.c_int, ip, C.POINTER(C.c_int64), ip, C.POINTER(C.c_int64),
                                C.POINTER(C.c_int64), vp, vp, C.c_int], C.c_int),
        "maus_pop_draw_min_len": ([], C.c_int),
        "maus_spmm_set_method": ([vp, C.c_int, C.c_int], C.c_int),
        "maus_spmm_get_method": ([vp], C.c_int),
        "maus_spmm_kernel_for": ([vp, C.c_int], C.c_int),
        "maus_spmm_plan": ([C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, ip], C.c_int),
        "maus_spmm_sell_info": ([vp, C.c_int, ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64)], C.c_int),
        "maus_band_outer_nb": ([vp, C.c_int, C.c_int, C.c_int], C.c_int),
        "maus_band_plan": ([C.c_int, C.c_int, C.c_int, C.c_int, i32p, i32p, i32p, C.POINTER(C.c_int64)], C.c_int),
        "maus_band_set_split": ([vp, C.c_int, C.c_int], C.c_int),
        "maus_band_get_split": ([vp, ip], C.c_int),
        "maus_band_set_real": ([vp, C.c_int], C.c_int),
        "maus_band_get_real": ([vp], C.c_int),
        "maus_band_real_plan": ([vp, C.c_int, C.c_int, vp, vp], C.c_int),
        "maus_band_real_kinds": ([C.c_int] * 6 + [vp], C.c_int),
        "maus_band_split_plan": ([C.c_int] * 5 + [i32p] * 6 + [C.POINTER(C.c_int64)], C.c_int),
        "maus_device_count": ([], C.c_int),
        "maus_comm_unique_id": ([C.c_char_p], C.c_int),
        "maus_comm_init": ([vp, C.c_int, C.c_int, C.c_char_p], C.c_int),
        "maus_comm_destroy": ([vp], C.c_int),
        "maus_comm_info": ([vp, ip, ip], C.c_int),
        "maus_comm_allgather_records": ([vp, vp, C.c_size_t, vp], C.c_int),
        "maus_comm_allgather_rows": ([vp, C.c_int, vp, vp, C.c_int], C.c_int),
        "maus_comm_bcast": ([vp, vp, C.c_size_t, C.c_int], C.c_int),
        "maus_comm_bcast_eigvecs": ([vp, C.c_int, C.c_int], C.c_int),
        "maus_comm_set_matrix": ([vp, vp, C.c_int, C.c_int, C.c_int], C.c_int),
        "maus_comm_stats": ([vp, C.POINTER(C.c_long), dp, dp, C.c_int], C.c_int),
    }
    for name, (args, res) in sig.items():
        fn = getattr(lib, name)          # AttributeError here == missing export: fail loudly
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


def _c128(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.complex128)
    if shape is not None:
        assert a.shape == tuple(shape), (a.shape, shape)
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _ClosedLib:
    """Stands in for the library handle of a closed Context: any call raises instead of handing a NULL context to C."""

    def __getattr__(self, name):
        raise MausHipError(f"{name}: the context has been closed")


class Context:
    """One device context (one per GPU).  Thin, typed wrappers over the C ABI."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.maus_ctx_create(device, C.byref(h))
        if rc != 0 or not h:
            msg = self.lib.maus_last_error(None)
            raise MausHipError(f"maus_ctx_create(device={device}) failed: {msg.decode() if msg else rc}; "
                               "a MI355X (gfx950) device is required -- no CPU fallback exists")
        self.h = h
        self.device = device
        self.rows = self.cols = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.maus_ctx_destroy(self.h)
            self.h = None
            self.lib = _ClosedLib()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if not getattr(self, "h", None):
            raise MausHipError(f"{what}: the context has been closed")
        if rc != 0:
            msg = self.lib.maus_last_error(self.h)
            raise MausHipError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")

    # -- info / measurement ------------------------------------------------
    def device_info(self):
        name = C.create_string_buffer(256)
        cus = C.c_int()
        tot, fr = C.c_size_t(), C.c_size_t()
        self._ck(self.lib.maus_device_info(self.h, name, 256, C.byref(cus), C.byref(tot), C.byref(fr)), "maus_device_info")
        return {"name": name.value.decode(), "cus": cus.value, "hbm_total": tot.value, "hbm_free": fr.value}

    def sync(self):
        self._ck(self.lib.maus_sync(self.h), "maus_sync")

    def timer_start(self):
        self._ck(self.lib.maus_timer_start(self.h), "maus_timer_start")

    def timer_stop(self) -> float:
        ms = C.c_float()
        self._ck(self.lib.maus_timer_stop(self.h, C.byref(ms)), "maus_timer_stop")
        return float(ms.value)

    def profile_enable(self, on=True):
        self._ck(self.lib.maus_profile_enable(self.h, int(on)), "maus_profile_enable")

    def profile_read_class(self, k):
        n = C.c_int()
        ms, fl, by, un = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        self._ck(self.lib.maus_profile_read(self.h, k, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)), "maus_profile_read")
        self._ck(self.lib.maus_profile_union_ms(self.h, k, C.byref(un)), "maus_profile_union_ms")
        return {"launches": n.value, "ms": ms.value, "flops": fl.value, "bytes": by.value, "union_ms": un.value}

    def profile_read(self):
        prof = {name: self.profile_read_class(k) for k, name in enumerate(KC_NAMES)}
        prof["band_split"] = self.profile_read_class(KC_BAND_SPLIT)
        prof["gmres_real"] = self.profile_read_class(KC_GMRES_REAL)
        prof["spmm_real"] = self.profile_read_class(KC_SPMM_REAL)
        prof["band_real"] = self.profile_read_class(KC_BAND_REAL)
        return prof

    def lu_workspace_allocations(self) -> int:
        return int(self.lib.maus_lu_workspace_allocs(self.h))

    def set_shared_device(self, shared=True):
        """Tell the library that other processes use this GPU too (ranks of a gloo rehearsal on one device): kernels that
        need every one of their workgroups resident at once (the multi-workgroup LU panel) are then never used."""
        self._ck(self.lib.maus_set_shared_device(self.h, 1 if shared else 0), "maus_set_shared_device")

    def lu_max_n(self) -> int:
        """Largest n the direct LU path and both GMRES modes accept in this build of the library."""
        return int(self.lib.maus_lu_max_n())

    def lu_mw_aborts(self) -> int:
        """Batches that were repeated with one panel workgroup per matrix after a rendezvous time-out."""
        return int(self.lib.maus_lu_mw_aborts(self.h))

    # -- problem data --------------------------------------------------------
    def set_matrix(self, A):
        A = _c128(A)
        assert A.ndim == 2
        self.rows, self.cols = A.shape
        self._ck(self.lib.maus_set_matrix(self.h, _ptr(A), A.shape[0], A.shape[1]), "maus_set_matrix")

    def set_matrix_csr(self, A):
        """Upload a scipy.sparse matrix (any format) as complex CSR with sorted, summed indices (maus_set_matrix_csr);
        the library keeps no dense copy.  Raw arrays go straight to set_matrix_csr_arrays."""
        import scipy.sparse as sp
        M = sp.csr_matrix(A, dtype=np.complex128, copy=True)
        M.sum_duplicates()
        M.sort_indices()
        self.set_matrix_csr_arrays(M.shape[0], M.shape[1], M.indptr, M.indices, M.data)

    def set_matrix_csr_arrays(self, rows, cols, indptr, indices, values):
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        values = _c128(values)
        nnz = int(values.shape[0])
        if indptr.shape != (int(rows) + 1,) or indices.shape != (nnz,):
            raise MausHipError(f"maus_set_matrix_csr: array lengths (indptr {indptr.shape}, indices {indices.shape}, "
                               f"values {values.shape}) do not fit rows = {rows}, nnz = {nnz}")
        self._ck(self.lib.maus_set_matrix_csr(self.h, int(rows), int(cols), nnz, _ptr(indptr), _ptr(indices), _ptr(values)),
                 "maus_set_matrix_csr")
        self.rows, self.cols = int(rows), int(cols)

    def matrix_is_sparse(self):
        """None for a dense matrix, else the SpMM schedule chosen at bind time ('rows' or 'wave')."""
        return SPMM_SCHEDULES[int(self.lib.maus_matrix_is_sparse(self.h))]

    def set_rhs(self, b):
        b = _c128(b)
        self._ck(self.lib.maus_set_rhs(self.h, _ptr(b), b.shape[0]), "maus_set_rhs")

    def set_eigvecs(self, V):
        V = _c128(V)
        self._ck(self.lib.maus_set_eigvecs(self.h, _ptr(V), V.shape[0]), "maus_set_eigvecs")

    def get_eigvecs(self):
        n = self.rows
        V = np.empty((n, n), dtype=np.complex128)
        self._ck(self.lib.maus_get_eigvecs(self.h, _ptr(V), n), "maus_get_eigvecs")
        return V

    # -- population ----------------------------------------------------------
    def pop_reserve(self, cap):
        self._ck(self.lib.maus_pop_reserve(self.h, int(cap)), "maus_pop_reserve")

    def pop_capacity(self):
        return self.lib.maus_pop_capacity(self.h)

    @staticmethod
    def _slots(slots):
        return np.ascontiguousarray(slots, dtype=np.int32)

    def pop_put(self, which, slots, vecs):
        s = self._slots(slots)
        v = _c128(vecs)
        if v.ndim == 1:
            v = v[None, :]
        assert v.shape[0] == s.shape[0]
        self._ck(self.lib.maus_pop_put(self.h, which, _ptr(s), s.shape[0], _ptr(v), v.shape[1]), "maus_pop_put")

    def pop_get(self, which, slots, length):
        s = self._slots(slots)
        out = np.empty((s.shape[0], length), dtype=np.complex128)
        self._ck(self.lib.maus_pop_get(self.h, which, _ptr(s), s.shape[0], _ptr(out), length), "maus_pop_get")
        return out

    def pop_draw(self, which, length, slots, kinds, scale, state, ordinals, substreams=0):
        """Rows `slots` of population array `which` drawn on the device from the legacy NumPy stream (maus_pop_draw): draw k
        is the pair np.random.rand(length) + 1j*np.random.rand(length) number ordinals[k] counted from `state`
        (np.random.get_state()), of kind kinds[k] (DRAW_RAW / DRAW_UNIT / DRAW_NORM) and scale[k] (None: 1.0).  Returns the
        norms.  The caller advances its own stream."""
        s = self._slots(slots)
        k = s.shape[0]
        kd = np.ascontiguousarray(kinds, dtype=np.int32)
        ords = np.ascontiguousarray(ordinals, dtype=np.int32)
        assert kd.shape == (k,) and ords.shape == (k,)
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
        assert sc is None or sc.shape == (k,)
        pd = MtDesc()
        C.memmove(pd.key, np.ascontiguousarray(state[1], dtype=np.uint32).ctypes.data, 624 * 4)
        pd.pos = int(state[2]); pd.words_per_candidate = 4 * int(length); pd.lead_words = 0
        pd.ordinals = ords.ctypes.data_as(C.POINTER(C.c_int32))
        norms = np.zeros(k, dtype=np.float64)
        self._ck(self.lib.maus_pop_draw(self.h, int(which), int(length), k, _ptr(s), _ptr(kd), None if sc is None else _ptr(sc),
                                        C.cast(C.pointer(pd), C.c_void_p), int(substreams), _ptr(norms)), "maus_pop_draw")
        return norms

    def pop_draw_min_len(self) -> int:
        return int(self.lib.maus_pop_draw_min_len())

    def pop_copy(self, which_dst, which_src, slots):
        s = self._slots(slots)
        self._ck(self.lib.maus_pop_copy(self.h, int(which_dst), int(which_src), _ptr(s), s.shape[0]), "maus_pop_copy")

    def pop_device_ptr(self, which):
        """(device address, leading dimension in complex elements, capacity in rows) of a population array."""
        ptr, ld, cap = C.c_void_p(), C.c_long(), C.c_int()
        self._ck(self.lib.maus_pop_device_ptr(self.h, int(which), C.byref(ptr), C.byref(ld), C.byref(cap)), "maus_pop_device_ptr")
        return int(ptr.value), int(ld.value), int(cap.value)

    def hist_append(self, which, slots, length) -> int:
        """Append rows `slots` of population array `which` to the device history; returns the first row's index."""
        s = self._slots(slots)
        first = C.c_int64()
        self._ck(self.lib.maus_hist_append(self.h, int(which), _ptr(s), s.shape[0], int(length), C.byref(first)), "maus_hist_append")
        return int(first.value)

    def hist_get(self, indices, length):
        ix = np.ascontiguousarray(indices, dtype=np.int64)
        out = np.empty((ix.shape[0], length), dtype=np.complex128)
        self._ck(self.lib.maus_hist_get(self.h, _ptr(ix), ix.shape[0], int(length), _ptr(out)), "maus_hist_get")
        return out

    def hist_clear(self):
        self._ck(self.lib.maus_hist_clear(self.h), "maus_hist_clear")

    def hist_generation(self) -> int:
        if not getattr(self, "h", None):
            raise MausHipError("maus_hist_generation: the context has been closed")
        return int(self.lib.maus_hist_generation(self.h))

    # -- phases --------------------------------------------------------------
    def matvec_rayleigh(self, slots):
        s = self._slots(slots)
        num = np.empty(s.shape[0], dtype=np.complex128)
        den = np.empty(s.shape[0], dtype=np.complex128)
        self._ck(self.lib.maus_matvec_rayleigh(self.h, _ptr(s), s.shape[0], _ptr(num), _ptr(den)), "maus_matvec_rayleigh")
        return num, den

    def _pert_arg(self, k, pert_mode, pert_data):
        """(keep-alive objects, void*) for the pert_data argument of the solve entry points."""
        if pert_mode == PERT_UNIFORM:
            pd = np.ascontiguousarray(pert_data, dtype=np.float64)
            assert pd.shape == (k, 2, self.rows, self.rows), pd.shape
            return (pd,), _ptr(pd)
        if pert_mode == PERT_MT19937:
            # pert_data = (numpy_state, words_per_candidate, lead_words, ordinals)
            st, wpc, lead, ords = pert_data
            ords = np.ascontiguousarray(ords, dtype=np.int32)
            assert ords.shape == (k,)
            pd = MtDesc()
            C.memmove(pd.key, np.ascontiguousarray(st[1], dtype=np.uint32).ctypes.data, 624 * 4)
            pd.pos = int(st[2]); pd.words_per_candidate = int(wpc); pd.lead_words = int(lead)
            pd.ordinals = ords.ctypes.data_as(C.POINTER(C.c_int32))
            return (pd, ords), C.cast(C.pointer(pd), C.c_void_p)
        return (), None

    def shifted_lu_solve(self, slots, shift, psi, rhs_mode=0, pert_mode=PERT_NONE, pert_data=None):
        s = self._slots(slots)
        k = s.shape[0]
        sh = _c128(shift, (k,))
        ps = np.ascontiguousarray(psi, dtype=np.float64)
        assert ps.shape == (k,)
        status = np.zeros(k, dtype=np.int32)
        keep, pdp = self._pert_arg(k, pert_mode, pert_data)
        self._ck(self.lib.maus_shifted_lu_solve(self.h, _ptr(s), k, _ptr(sh), _ptr(ps), int(rhs_mode), int(pert_mode),
                                                pdp, _ptr(status)), "maus_shifted_lu_solve")
        return status

    def lu_reserve(self, n, count) -> int:
        """Size the LU workspace once for `count` simultaneous n x n solves; returns its capacity in matrices."""
        cap = C.c_int()
        self._ck(self.lib.maus_lu_reserve(self.h, int(n), int(count), C.byref(cap)), "maus_lu_reserve")
        return int(cap.value)

    def relax_normalise(self, slots, alpha, normalise=True):
        s = self._slots(slots)
        al = _c128(alpha, (s.shape[0],))
        nrm = np.empty(s.shape[0], dtype=np.float64)
        self._ck(self.lib.maus_relax_normalise(self.h, _ptr(s), s.shape[0], _ptr(al), 1 if normalise else 0, _ptr(nrm)),
                 "maus_relax_normalise")
        return nrm

    def residual(self, kind, slots, lam=None):
        s = self._slots(slots)
        l = None if lam is None else _c128(lam, (s.shape[0],))
        res = np.empty(s.shape[0], dtype=np.float64)
        fin = np.empty(s.shape[0], dtype=np.int32)
        self._ck(self.lib.maus_residual(self.h, int(kind), _ptr(s), s.shape[0], _ptr(l), _ptr(res), _ptr(fin)), "maus_residual")
        return res, fin.astype(bool)

    def svd_power_step(self, slots):
        s = self._slots(slots)
        norms = np.empty((s.shape[0], 4), dtype=np.float64)
        self._ck(self.lib.maus_svd_power_step(self.h, _ptr(s), s.shape[0], _ptr(norms)), "maus_svd_power_step")
        return norms

    def herm_tridiag(self):
        """A = Q T Q^H of the bound Hermitian matrix on the device (zhetrd semantics): (d[n], e[n-1]) of the real T."""
        n = self.rows
        d = np.empty(n, dtype=np.float64)
        e = np.empty(max(n - 1, 1), dtype=np.float64)
        self._ck(self.lib.maus_herm_tridiag(self.h, _ptr(d), _ptr(e)), "maus_herm_tridiag")
        return d, e[: n - 1]

    @staticmethod
    def _scaled_tridiagonal(d, e):
        d = np.ascontiguousarray(d, dtype=np.float64)
        e = np.ascontiguousarray(e, dtype=np.float64)
        n = d.shape[0]
        if e.shape[0] != max(n - 1, 0):
            raise ValueError("tridiagonal matrix: e must have n - 1 entries")
        if not (np.isfinite(d).all() and np.isfinite(e).all()):    # (max(t, nan) is t: a NaN in e alone would pass a test of t)
            raise ValueError("tridiagonal matrix is not finite")
        t = max(float(np.max(np.abs(d))) if n else 0.0, float(np.max(np.abs(e))) if n > 1 else 0.0)
        s = 2.0 ** int(np.floor(np.log2(t))) if t > 0.0 else 1.0           # a power of two: the scaling is exact
        return n, d / s, np.ascontiguousarray(e / s if n > 1 else np.zeros(1)), s

    def herm_set_chunk(self, tiles):
        """Tiles per workgroup of the reduction's matvec: 0 (the rule, the default), 4, 8 or 16 for every column (tests, timing)."""
        self._ck(self.lib.maus_herm_set_chunk(self.h, int(tiles)), "maus_herm_set_chunk")

    @staticmethod
    def herm_chunk_plan(n, i, forced=0):
        """(T, hch, ns) that column i of an order-n reduction launches under `forced` (maus_herm_chunk_plan): block rows of the
        tile grid, tiles per workgroup, tile workgroups.  Needs neither a context nor a device."""
        T, hch, ns = C.c_int(0), C.c_int(0), C.c_int(0)
        if load_library().maus_herm_chunk_plan(int(n), int(i), int(forced), C.byref(T), C.byref(hch), C.byref(ns)) != 0:
            raise MausHipError(f"maus_herm_chunk_plan: bad order, column or chunk ({n}, {i}, {forced})")
        return T.value, hch.value, ns.value

    def herm_release(self):
        """Hand back the reflector store of herm_tridiag (n x n) when no back-transformation will follow."""
        self._ck(self.lib.maus_herm_release(self.h), "maus_herm_release")

    def herm_tridiag_eigvals(self, d, e):
        """Eigenvalues (ascending) of the real symmetric tridiagonal T = (d, e) by bisection on the device."""
        n, ds, es, s = self._scaled_tridiagonal(d, e)
        w = np.empty(n, dtype=np.float64)
        self._ck(self.lib.maus_herm_tridiag_eigvals(self.h, _ptr(ds), _ptr(es), n, _ptr(w)), "maus_herm_tridiag_eigvals")
        return w * s

    def herm_tridiag_eig(self, d, e):
        """Eigenvalues (ascending) of the real symmetric tridiagonal T = (d, e) by bisection on the device, its eigenvectors
        (twisted factorisation, no reorthogonalisation) left there for herm_backtransform(None).  Returns (w, diag) with diag =
        (smallest gap / ||T||, largest residual component / ||T||, ||T||): see engine.device_eigh for the acceptance rule.
        T is scaled by a power of two to ||T|| ~ 1 first (exact), so the squares of the off-diagonal stay in range."""
        n, ds, es, s = self._scaled_tridiagonal(d, e)
        w = np.empty(n, dtype=np.float64)
        diag = np.empty(3, dtype=np.float64)
        self._ck(self.lib.maus_herm_tridiag_eig(self.h, _ptr(ds), _ptr(es), n, _ptr(w), _ptr(diag)), "maus_herm_tridiag_eig")
        return w * s, (float(diag[0]), float(diag[1]), float(diag[2]) * s)

    def herm_backtransform(self, Z):
        """V = Q Z on the device from the real eigenvectors Z[n][n] of T (None: those herm_tridiag_eig left on the device); V
        becomes the context's eigenvector matrix.  A column-major Z (what LAPACK returns) is passed as it is and transposed on
        the device."""
        if Z is None:
            self._ck(self.lib.maus_herm_backtransform(self.h, None, 0), "maus_herm_backtransform")
            return
        Z = np.asarray(Z, dtype=np.float64)
        if Z.shape != (self.rows, self.rows):
            raise ValueError("herm_backtransform: Z must be n x n")
        if Z.flags.f_contiguous and not Z.flags.c_contiguous:
            self._ck(self.lib.maus_herm_backtransform(self.h, _ptr(Z.T), 1), "maus_herm_backtransform")
        else:
            Z = np.ascontiguousarray(Z)
            self._ck(self.lib.maus_herm_backtransform(self.h, _ptr(Z), 0), "maus_herm_backtransform")

    def svd_power_propose(self, slots):
        """The power step without its effect: norms as svd_power_step, proposed u / v left in POP_Y / POP_W."""
        s = self._slots(slots)
        norms = np.empty((s.shape[0], 4), dtype=np.float64)
        self._ck(self.lib.maus_svd_power_propose(self.h, _ptr(s), s.shape[0], _ptr(norms)), "maus_svd_power_propose")
        return norms

    def svd_commit(self, slots):
        s = self._slots(slots)
        if s.shape[0]:
            self._ck(self.lib.maus_svd_commit(self.h, _ptr(s), s.shape[0]), "maus_svd_commit")

    def herm_match(self, slots):
        s = self._slots(slots)
        idx = np.empty(s.shape[0], dtype=np.int32)
        nrm = np.empty(s.shape[0], dtype=np.float64)
        self._ck(self.lib.maus_herm_match(self.h, _ptr(s), s.shape[0], _ptr(idx), _ptr(nrm)), "maus_herm_match")
        return idx, nrm

    # -- thick-restart Lanczos of the sparse Hermitian shortcut (csrc/lanczos.hip) ---------------------------------------
    def lanczos_begin(self, v0, ncv):
        """Room for a basis of ncv + 1 rows on the device; row 0 = v0 / ||v0||."""
        v = _c128(v0, (self.rows,))
        self._ck(self.lib.maus_lanczos_begin(self.h, _ptr(v), int(ncv)), "maus_lanczos_begin")

    def lanczos_inject(self, j, v):
        """Row j = v, orthogonalised against rows 0 .. j - 1 and normalised (continuation after a breakdown)."""
        v = _c128(v, (self.rows,))
        self._ck(self.lib.maus_lanczos_inject(self.h, int(j), _ptr(v)), "maus_lanczos_inject")

    def lanczos_extend(self, j0, j1, tol_abs):
        """Lanczos steps j0 .. j1 - 1 with full reorthogonalisation -> (alpha[j1 - j0], beta[j1 - j0]); a step whose beta
        is not above tol_abs leaves a zero row."""
        alpha = np.empty(j1 - j0, dtype=np.float64)
        beta = np.empty(j1 - j0, dtype=np.float64)
        self._ck(self.lib.maus_lanczos_extend(self.h, int(j0), int(j1), float(tol_abs), _ptr(alpha), _ptr(beta)),
                 "maus_lanczos_extend")
        return alpha, beta

    def lanczos_restart(self, S):
        """Thick restart: rows 0 .. keep - 1 <- S^T rows 0 .. m - 1 for the real S[m, keep]; row keep <- row m."""
        S = np.ascontiguousarray(S, dtype=np.float64)
        self._ck(self.lib.maus_lanczos_restart(self.h, _ptr(S), S.shape[0], S.shape[1]), "maus_lanczos_restart")

    def lanczos_finish(self, S):
        """The k Ritz rows S^T rows 0 .. m - 1 for the real S[m, k] stay resident (herm_match_rows); the basis is freed."""
        S = np.ascontiguousarray(S, dtype=np.float64)
        self._ck(self.lib.maus_lanczos_finish(self.h, _ptr(S), S.shape[0], S.shape[1]), "maus_lanczos_finish")
        self._ritz_k = int(S.shape[1])

    def herm_match_rows(self, slots):
        s = self._slots(slots)
        idx = np.empty(s.shape[0], dtype=np.int32)
        nrm = np.empty(s.shape[0], dtype=np.float64)
        self._ck(self.lib.maus_herm_match_rows(self.h, _ptr(s), s.shape[0], _ptr(idx), _ptr(nrm)), "maus_herm_match_rows")
        return idx, nrm

    def get_ritz_rows(self):
        """The resident Ritz rows, k x n, ascending in lambda."""
        k = int(getattr(self, "_ritz_k", 0))
        out = np.empty((k, self.rows), dtype=np.complex128)
        self._ck(self.lib.maus_get_ritz_rows(self.h, _ptr(out), k, self.rows), "maus_get_ritz_rows")
        return out

    def lanczos_get_basis(self, j0, count):
        """Rows j0 .. j0 + count - 1 of the live Lanczos basis, count x n (read-only; tests)."""
        out = np.empty((max(int(count), 0), self.rows), dtype=np.complex128)
        self._ck(self.lib.maus_lanczos_get_basis(self.h, int(j0), int(count), _ptr(out)), "maus_lanczos_get_basis")
        return out

    def gram(self, which, slots, length):
        """G[i, j] = np.vdot(x_i, x_j) for the rows `slots` of population array `which` (first `length` entries)."""
        s = self._slots(slots)
        k = s.shape[0]
        out = np.empty((k, k), dtype=np.complex128)
        self._ck(self.lib.maus_gram(self.h, int(which), _ptr(s), k, int(length), _ptr(out)), "maus_gram")
        return out

    def gmres(self, slots, shift, psi, rhs_mode, use_jacobi, rtol=1e-8, restart=20, maxiter=50):
        s = self._slots(slots)
        k = s.shape[0]
        sh = _c128(shift, (k,))
        ps = np.ascontiguousarray(psi, dtype=np.float64)
        uj = np.ascontiguousarray(use_jacobi, dtype=np.int32)
        info = np.zeros(k, dtype=np.int32)
        inner = np.zeros(k, dtype=np.int32)
        status = np.zeros(k, dtype=np.int32)
        self._ck(self.lib.maus_gmres(self.h, _ptr(s), k, _ptr(sh), _ptr(ps), int(rhs_mode), _ptr(uj), float(rtol),
                                     int(restart), int(maxiter), _ptr(info), _ptr(inner), _ptr(status)), "maus_gmres")
        return info, inner, status

    def gmres_pert(self, slots, shift, psi, rhs_mode, want_jacobi, pert_mode, pert_data, rtol=1e-8, restart=20, maxiter=50):
        """GMRES against the materialised H_k including the random term of AMS:49-50 -> (info, inner, status, jacobi_used)."""
        s = self._slots(slots)
        k = s.shape[0]
        sh = _c128(shift, (k,))
        ps = np.ascontiguousarray(psi, dtype=np.float64)
        wj = np.ascontiguousarray(want_jacobi, dtype=np.int32)
        info = np.zeros(k, dtype=np.int32)
        inner = np.zeros(k, dtype=np.int32)
        status = np.zeros(k, dtype=np.int32)
        jac = np.zeros(k, dtype=np.int32)
        keep, pdp = self._pert_arg(k, pert_mode, pert_data)
        self._ck(self.lib.maus_gmres_pert(self.h, _ptr(s), k, _ptr(sh), _ptr(ps), int(rhs_mode), _ptr(wj), int(pert_mode), pdp,
                                          float(rtol), int(restart), int(maxiter), _ptr(info), _ptr(inner), _ptr(status),
                                          _ptr(jac)), "maus_gmres_pert")
        return info, inner, status, jac.astype(bool)

    def jacobi_check(self, shift, psi):
        sh = _c128(shift)
        k = sh.shape[0]
        ps = np.ascontiguousarray(psi, dtype=np.float64)
        ok = np.zeros(k, dtype=np.int32)
        self._ck(self.lib.maus_jacobi_check(self.h, k, _ptr(sh), _ptr(ps), _ptr(ok)), "maus_jacobi_check")
        return ok.astype(bool)

    # -- band solves of a sparse matrix (csrc/band.hip) ---------------------------------------------------------------
    def sparse_max_n(self) -> int:
        """Largest n of the CSR eigenvalue / linear path (band solves, GMRES on a CSR matrix)."""
        return int(self.lib.maus_sparse_max_n())

    def band_prepare(self, perm):
        """Bind the ordering `perm` (band.band_order) of the bound sparse matrix; returns (kl, ku) of A[perm][:, perm]."""
        p = np.ascontiguousarray(perm, dtype=np.int32)
        kl, ku = C.c_int(), C.c_int()
        self._ck(self.lib.maus_band_prepare(self.h, _ptr(p), int(p.shape[0]), C.byref(kl), C.byref(ku)), "maus_band_prepare")
        return int(kl.value), int(ku.value)

    def band_reserve(self, count) -> int:
        """Size the band workspace once for `count` simultaneous solves; returns its capacity in solves."""
        cap = C.c_int()
        self._ck(self.lib.maus_band_reserve(self.h, int(count), C.byref(cap)), "maus_band_reserve")
        return int(cap.value)

    def band_solve(self, slots, shift, psi, rhs_mode=0):
        """shifted_lu_solve (pert_mode NONE) through the band LU of the bound ordering: W[slot] = (A - shift I + psi I)^-1 rhs."""
        s = self._slots(slots)
        k = s.shape[0]
        sh = _c128(shift, (k,))
        ps = np.ascontiguousarray(psi, dtype=np.float64)
        assert ps.shape == (k,)
        status = np.zeros(k, dtype=np.int32)
        self._ck(self.lib.maus_band_solve(self.h, _ptr(s), k, _ptr(sh), _ptr(ps), int(rhs_mode), _ptr(status)), "maus_band_solve")
        return status

    def band_workspace_allocations(self) -> int:
        return int(self.lib.maus_band_workspace_allocs(self.h))

    def band_set_method(self, method):
        """The kernels of the band entry points: BAND_COLUMN (the default), BAND_BLOCKED, BAND_TILED, BAND_WIDE or
        BAND_NARROW; kept across matrices."""
        self._ck(self.lib.maus_band_set_method(self.h, int(method)), "maus_band_set_method")

    def band_method(self) -> int:
        return int(self.lib.maus_band_get_method(self.h))

    def band_set_split(self, on, part_len=0):
        """The split beside the method (maus_band_set_split): on / off, part_len 0 for the rule or a forced partition length
        (at least 2 (kl + ku) + 2, checked where a band is solved); kept across matrices."""
        self._ck(self.lib.maus_band_set_split(self.h, int(bool(on)) if isinstance(on, bool) else int(on), int(part_len)),
                 "maus_band_set_split")

    def band_split(self):
        """(on, forced partition length or 0) of maus_band_set_split."""
        m = C.c_int()
        on = self.lib.maus_band_get_split(self.h, C.byref(m))
        self._ck(min(on, 0), "maus_band_get_split")
        return bool(on), int(m.value)

    def band_set_real(self, mode):
        """Real arithmetic for the band solves of a real sparse system (maus_band_set_real): BAND_REAL_OFF, or BAND_REAL_ON (a
        band_solve() call whose CSR operand, b and shifts all have imaginary parts of +-0, with rhs_mode 1, under the column
        kernel or the narrow method, with or without the split, runs on band storage of doubles; the complex path's x, ipiv
        and status; csrc/band.hip).  Every other call runs complex as ever.  band_lu() follows it for arrays whose imaginary
        parts are all +-0.  Independent of real_set_method(); kept across matrices."""
        self._ck(self.lib.maus_band_set_real(self.h, int(mode)), "maus_band_set_real")

    def band_real(self) -> int:
        return int(self.lib.maus_band_get_real(self.h))

    def band_real_plan(self, rhs_mode, shift) -> dict:
        """What a band_solve() call with this rhs_mode and these shifts does on the bound matrix, ordering and b
        (maus_band_real_plan, the function band_solve() itself decides by): 'real' (bool), 'why' (BAND_REAL_OK or the first
        condition of the rule that fails), 'kind' (BAND_COLUMN ...; as band_kernel_for) and 'split' (bool)."""
        sh = _c128(np.atleast_1d(np.asarray(shift, dtype=np.complex128)))
        out = np.zeros(4, dtype=np.int32)
        self._ck(self.lib.maus_band_real_plan(self.h, int(rhs_mode), int(sh.shape[0]), _ptr(sh), _ptr(out)), "maus_band_real_plan")
        return {"real": bool(out[0]), "why": int(out[1]), "kind": int(out[2]), "split": bool(out[3])}

    def band_kernel_for(self, n, kl, ku):
        """(kernel, nb) that an (n, kl, ku) band runs under the current method: (BAND_COLUMN, 1), (BAND_BLOCKED, nb),
        (BAND_TILED, nb), (BAND_WIDE, nb of the inner steps) or (BAND_NARROW, 1)."""
        nb = C.c_int()
        k = self.lib.maus_band_kernel_for(self.h, int(n), int(kl), int(ku), C.byref(nb))
        self._ck(min(k, 0), "maus_band_kernel_for")
        return int(k), int(nb.value)

    def band_outer_nb(self, n, kl, ku) -> int:
        """Width of the outer block (64) where an (n, kl, ku) band runs the wide method under the current method, else 0."""
        k = self.lib.maus_band_outer_nb(self.h, int(n), int(kl), int(ku))
        self._ck(min(k, 0), "maus_band_outer_nb")
        return int(k)

    def gmres_set_method(self, method):
        """The schedule of gmres()'s post step for a CSR-bound matrix: GMRES_DEFAULT (one workgroup per candidate) or GMRES_WIDE
        (n split over workgroups, csrc/gmres.hip); dense matrices and gmres_pert ignore it.  Kept across matrices."""
        self._ck(self.lib.maus_gmres_set_method(self.h, int(method)), "maus_gmres_set_method")

    def gmres_method(self) -> int:
        return int(self.lib.maus_gmres_get_method(self.h))

    def gmres_kernel_for(self, n, csr) -> int:
        """What the post step of an n x n matrix (csr: CSR-bound) runs under the current method: 0 a register kernel, 1 the
        stream kernel, 2 the wide step."""
        k = self.lib.maus_gmres_kernel_for(self.h, int(n), int(bool(csr)))
        self._ck(min(k, 0), "maus_gmres_kernel_for")
        return int(k)

    def real_set_method(self, method):
        """Real arithmetic for gmres() on a real sparse system: REAL_OFF, or REAL_ON (a call whose CSR operand, b and shifts all
        have imaginary parts of +-0 runs on rows of doubles with real copies of the operand, the diagonal and b; the complex
        path's bits; csrc/gmres.hip).  Every other call runs complex as ever.  Kept across matrices."""
        self._ck(self.lib.maus_real_set_method(self.h, int(method)), "maus_real_set_method")

    def real_method(self) -> int:
        return int(self.lib.maus_real_get_method(self.h))

    def real_plan(self, rhs_mode, shift) -> dict:
        """What a gmres() call with this rhs_mode and these shifts does on the bound matrix and b (maus_real_plan, the function
        gmres() itself decides by): 'real' (bool), 'why' (REAL_OK or the first condition of the rule that fails), 'post' (0
        register kernel, 1 stream kernel, 2 wide step; -1 without a square CSR matrix), 'spmm' (SPMM_KERNEL_*), 'allocs' (real
        copies allocated on this context so far) and 'bytes' (of the real copies held now)."""
        sh = _c128(np.atleast_1d(np.asarray(shift, dtype=np.complex128)))
        out = np.zeros(6, dtype=np.int64)
        self._ck(self.lib.maus_real_plan(self.h, int(rhs_mode), int(sh.shape[0]), _ptr(sh), _ptr(out)), "maus_real_plan")
        return {"real": bool(out[0]), "why": int(out[1]), "post": int(out[2]), "spmm": int(out[3]), "allocs": int(out[4]),
                "bytes": int(out[5])}

    def real_spmm(self, slots):
        """Y[slot] = A Re(X[slot]) by the SpMM kernels of the real path, imaginary part +0.0 (maus_real_spmm)."""
        s = self._slots(slots)
        self._ck(self.lib.maus_real_spmm(self.h, _ptr(s), s.shape[0]), "maus_real_spmm")

    def few_rows_set_method(self, method, slices=0):
        """Dense population products of at most 32 rows (A X, A^H u, conj(X) V, Gram blocks): FEW_ROWS_DEFAULT, or FEW_ROWS_SPLITK
        (K cut into slices over the whole device, joined in a fixed order; csrc/zgemm.hip).  `slices` 0: the library's rule;
        1..32 force that many (tests, timing).  Kept across matrices."""
        self._ck(self.lib.maus_few_rows_set_method(self.h, int(method), int(slices)), "maus_few_rows_set_method")

    def few_rows_method(self) -> int:
        return int(self.lib.maus_few_rows_get_method(self.h))

    def few_rows_kernel_for(self, M, N, K, b_layout=1, conj_a=False, conj_b=False):
        """(kernel, S) of an M x N x K product under the current method: (0, 1) the default kernels, (1, S) split-K."""
        S = C.c_int()
        k = self.lib.maus_few_rows_kernel_for(self.h, int(M), int(N), int(K), int(b_layout), int(bool(conj_a)), int(bool(conj_b)), C.byref(S))
        self._ck(min(k, 0), "maus_few_rows_kernel_for")
        return int(k), int(S.value)

    def few_rows_workspace_allocs(self) -> int:
        return int(self.lib.maus_few_rows_workspace_allocs(self.h))

    def spmm_set_method(self, method, fill_cap_percent=0):
        """Products with a CSR-bound matrix: SPMM_CSR (the default), or SPMM_SELL (the lane-per-row kernel on a sliced-ELL copy of
        every operand whose padded size stays within `fill_cap_percent` of nnz; the CSR kernel's bits; csrc/spmm.hip).
        `fill_cap_percent` 0: the library's 200; 100..1000000 for tests and timing.  Kept across matrices; with a CSR matrix
        bound the copies are built or freed at once."""
        self._ck(self.lib.maus_spmm_set_method(self.h, int(method), int(fill_cap_percent)), "maus_spmm_set_method")

    def spmm_method(self) -> int:
        return int(self.lib.maus_spmm_get_method(self.h))

    def spmm_kernel_for(self, adjoint=False) -> int:
        """What a product with the bound matrix (adjoint: with A^H) runs under the current method: SPMM_KERNEL_NONE (no CSR
        matrix), SPMM_KERNEL_ROWS, SPMM_KERNEL_WAVE or SPMM_KERNEL_SELL."""
        k = self.lib.maus_spmm_kernel_for(self.h, int(bool(adjoint)))
        self._ck(min(k, 0), "maus_spmm_kernel_for")
        return int(k)

    def spmm_sell_info(self, adjoint=False):
        """(slices, padded slots, bytes) of the resident sliced-ELL copy of A (adjoint: of A^H); zeros without one."""
        ns, padded, by = C.c_int(), C.c_int64(), C.c_int64()
        self._ck(self.lib.maus_spmm_sell_info(self.h, int(bool(adjoint)), C.byref(ns), C.byref(padded), C.byref(by)), "maus_spmm_sell_info")
        return int(ns.value), int(padded.value), int(by.value)

    def band_lu(self, ab, b, kl, ku, method=None):
        """zgbtrf + zgbtrs on the device: ab[count, 2kl+ku+1, n] in LAPACK's band layout (SciPy's `ab`), b[count, n] ->
        (x[count, n], ipiv[count, n] 0-based as SciPy returns it, status[count]).  `method`: for this call only."""
        if method is not None:
            prev = self.band_method()
            self.band_set_method(method)
            try:
                return self.band_lu(ab, b, kl, ku)
            finally:
                self.band_set_method(prev)
        ab = _c128(ab)
        b = _c128(b)
        if ab.ndim == 2:
            ab, b = ab[None], b[None]
        cnt, ldab, n = ab.shape
        assert ldab == 2 * kl + ku + 1 and b.shape == (cnt, n)
        abt = np.ascontiguousarray(ab.transpose(0, 2, 1))
        x = np.empty((cnt, n), dtype=np.complex128)
        ipiv = np.zeros((cnt, n), dtype=np.int32)
        status = np.zeros(cnt, dtype=np.int32)
        self._ck(self.lib.maus_band_lu_host(self.h, cnt, n, int(kl), int(ku), _ptr(abt), _ptr(b), _ptr(x), _ptr(ipiv), _ptr(status)),
                 "maus_band_lu_host")
        return x, ipiv - 1, status

    # -- population sharding: RCCL collectives on this context's stream (csrc/comm.hip) -----------------------------
    def comm_init(self, rank: int, world: int, unique_id: bytes):
        assert len(unique_id) == COMM_ID_BYTES
        self._ck(self.lib.maus_comm_init(self.h, int(rank), int(world), unique_id), "maus_comm_init")

    def comm_destroy(self):
        self._ck(self.lib.maus_comm_destroy(self.h), "maus_comm_destroy")

    def comm_allgather_records(self, send: np.ndarray, world: int) -> np.ndarray:
        """send: C-contiguous array (any dtype) of the same shape on every rank -> array of shape (world,) + send.shape."""
        send = np.ascontiguousarray(send)
        out = np.empty((world,) + send.shape, dtype=send.dtype)
        self._ck(self.lib.maus_comm_allgather_records(self.h, _ptr(send), send.nbytes, _ptr(out)), "maus_comm_allgather_records")
        return out

    def comm_allgather_rows(self, which, slots_by_rank, length):
        counts = np.ascontiguousarray([len(s) for s in slots_by_rank], dtype=np.int32)
        flat = np.ascontiguousarray([s for sl in slots_by_rank for s in sl], dtype=np.int32)
        self._ck(self.lib.maus_comm_allgather_rows(self.h, int(which), _ptr(flat), _ptr(counts), int(length)), "maus_comm_allgather_rows")

    def comm_bcast(self, arr: np.ndarray, root=0):
        """In-place broadcast of a C-contiguous array (same shape / dtype on every rank)."""
        assert arr.flags["C_CONTIGUOUS"]
        self._ck(self.lib.maus_comm_bcast(self.h, _ptr(arr), arr.nbytes, int(root)), "maus_comm_bcast")
        return arr

    def comm_set_matrix(self, A, rank, root=0, resident_on_root=False):
        """set_matrix of a sharded run: `root` uploads A (or, resident_on_root, broadcasts the copy its device already
        holds), the other ranks receive it device to device (only the shape of their A is read)."""
        upload = rank == root and not resident_on_root
        if upload:
            A = _c128(A)
        self._ck(self.lib.maus_comm_set_matrix(self.h, _ptr(A) if upload else None, A.shape[0], A.shape[1], int(root)),
                 "maus_comm_set_matrix")
        self.rows, self.cols = A.shape

    def comm_bcast_eigvecs(self, n, root=0):
        self._ck(self.lib.maus_comm_bcast_eigvecs(self.h, int(n), int(root)), "maus_comm_bcast_eigvecs")

    def comm_stats(self, reset=False):
        calls, by, ms = C.c_long(), C.c_double(), C.c_double()
        self._ck(self.lib.maus_comm_stats(self.h, C.byref(calls), C.byref(by), C.byref(ms), 1 if reset else 0), "maus_comm_stats")
        return {"collectives": int(calls.value), "bytes": float(by.value), "ms": float(ms.value)}

    # -- test / utility entry points ------------------------------------------
    def zgemm(self, A, B, C_in=None, b_layout=0, conj_a=False, conj_b=False, alpha=1.0, beta=0):
        A = _c128(A)
        B = _c128(B)
        M, K = A.shape
        N = B.shape[0] if b_layout else B.shape[1]
        Cm = np.zeros((M, N), dtype=np.complex128) if C_in is None else _c128(C_in).copy()
        self._ck(self.lib.maus_zgemm_host(self.h, M, N, K, _ptr(A), _ptr(B), _ptr(Cm), int(b_layout), int(conj_a),
                                          int(conj_b), float(alpha), int(beta)), "maus_zgemm_host")
        return Cm

    def lu_solve(self, A, b, want_ipiv=False):
        A = _c128(A)
        b = _c128(b)
        if A.ndim == 2:
            A = A[None]
            b = b[None]
        cnt, n, _ = A.shape
        x = np.empty((cnt, n), dtype=np.complex128)
        status = np.zeros(cnt, dtype=np.int32)
        ipiv = np.zeros((cnt, n), dtype=np.int32) if want_ipiv else None
        self._ck(self.lib.maus_lu_solve_host(self.h, cnt, n, _ptr(A), _ptr(b), _ptr(x), _ptr(status), _ptr(ipiv)), "maus_lu_solve_host")
        return (x, status, ipiv) if want_ipiv else (x, status)


def device_count() -> int:
    """HIP devices visible to this process (0 on a box without a GPU)."""
    return int(load_library().maus_device_count())


def band_plan(method, n, kl, ku):
    """(kind, nb, outer nb, workspace bytes per solve) of an (n, kl, ku) band under `method` (maus_band_plan): needs neither
    a context nor a device."""
    kind, nb, nbo, per = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    if load_library().maus_band_plan(int(method), int(n), int(kl), int(ku), C.byref(kind), C.byref(nb), C.byref(nbo), C.byref(per)) != 0:
        raise MausHipError(f"maus_band_plan: bad method or sizes ({method}, {n}, {kl}, {ku})")
    return int(kind.value), int(nb.value), int(nbo.value), int(per.value)


def band_split_plan(method, n, kl, ku, part_len=0):
    """(takes, partition length, partitions, n_red, kl_red, ku_red, bytes of the split's arrays per solve) of an (n, kl, ku)
    band under `method` and part_len (maus_band_split_plan): needs neither a context nor a device."""
    v = [C.c_int32() for _ in range(6)]
    per = C.c_int64()
    if load_library().maus_band_split_plan(int(method), int(n), int(kl), int(ku), int(part_len), *[C.byref(x) for x in v], C.byref(per)) != 0:
        raise MausHipError(f"maus_band_split_plan: bad method, sizes or partition length ({method}, {n}, {kl}, {ku}, {part_len})")
    return (bool(v[0].value),) + tuple(int(x.value) for x in v[1:]) + (int(per.value),)


def band_real_kinds(method, split, part_len, n, kl, ku):
    """(real, kind, split takes) of an (n, kl, ku) band under `method`, the split switch and part_len (maus_band_real_kinds):
    real says whether every kernel the solve would run has a real instantiation.  Needs neither a context nor a device."""
    out = np.zeros(3, dtype=np.int32)
    if load_library().maus_band_real_kinds(int(method), int(bool(split)), int(part_len), int(n), int(kl), int(ku), _ptr(out)) != 0:
        raise MausHipError(f"maus_band_real_kinds: bad method, sizes or partition length ({method}, {split}, {part_len}, {n}, {kl}, {ku})")
    return bool(out[0]), int(out[1]), bool(out[2])


def few_rows_plan(method, slices, M, N, K, b_layout=1, conj_a=False, conj_b=False):
    """(kernel, S) of an M x N x K population product under (method, slices) (maus_few_rows_plan): (0, 1) the default kernels,
    (1, S) split-K.  Needs neither a context nor a device."""
    S = C.c_int()
    k = load_library().maus_few_rows_plan(int(method), int(slices), int(M), int(N), int(K), int(b_layout), int(bool(conj_a)),
                                          int(bool(conj_b)), C.byref(S))
    if k < 0:
        raise MausHipError(f"maus_few_rows_plan: bad method, slices or sizes ({method}, {slices}, {M}, {N}, {K}, {b_layout})")
    return int(k), int(S.value)


def zgemm_plan(form, lu_tile, M, N, K, batch=1, b_layout=0, conj_a=False, conj_b=False):
    """(family, BM, BN) of an M x N x K product on `batch` matrices (maus_zgemm_plan): ZGEMM_4M, ZGEMM_3M or ZGEMM_3M_DMA and the
    workgroup tile, for the form ZGEMM_ROWS or ZGEMM_LU under the MAUS_LU_TILE mode `lu_tile` (arguments in the C order).  Needs neither a context nor a
    device."""
    bm, bn = C.c_int(), C.c_int()
    fam = load_library().maus_zgemm_plan(int(form), int(lu_tile), int(M), int(N), int(K), int(batch), int(b_layout),
                                         int(bool(conj_a)), int(bool(conj_b)), C.byref(bm), C.byref(bn))
    if fam < 0:
        raise MausHipError(f"maus_zgemm_plan: bad form, tile mode, sizes or layout ({form}, {lu_tile}, {M}, {N}, {K}, {batch}, {b_layout}, {conj_a}, {conj_b})")
    return int(fam), int(bm.value), int(bn.value)


def pop_draw_plan(length, ordinals, pos, substreams=0):
    """The generator plan of a maus_pop_draw call (maus_pop_draw_plan): a dict with S, E, ngen, the jump strides dj / dj2 in
    blocks of 624 words and the arrays extra / rpos, generator (k, sb, part) at index (k * S + sb) * 2 + part.  Needs neither
    a context nor a device."""
    lib = load_library()
    ords = np.ascontiguousarray(ordinals, dtype=np.int32)
    S, ngen = C.c_int(), C.c_int()
    E, dj, dj2 = C.c_int64(), C.c_int64(), C.c_int64()
    args = (int(length), int(ords.shape[0]), _ptr(ords), int(pos), int(substreams), C.byref(S), C.byref(E), C.byref(ngen), C.byref(dj), C.byref(dj2))
    if lib.maus_pop_draw_plan(*args, None, None, 0) != 0:
        raise MausHipError(f"maus_pop_draw_plan: bad length, count, ordinals, position or sub-stream count ({length}, {ords.shape[0]}, {pos}, {substreams})")
    extra = np.zeros(ngen.value, dtype=np.int32)
    rpos = np.zeros(ngen.value, dtype=np.int32)
    if lib.maus_pop_draw_plan(*args, _ptr(extra), _ptr(rpos), int(ngen.value)) != 0:
        raise MausHipError("maus_pop_draw_plan failed")
    return {"S": int(S.value), "E": int(E.value), "ngen": int(ngen.value), "dj": int(dj.value), "dj2": int(dj2.value), "extra": extra, "rpos": rpos}


def pop_draw_min_len() -> int:
    return int(load_library().maus_pop_draw_min_len())


def real_values_flagged(values) -> bool:
    """Whether the real path's rule counts these complex values as real: every imaginary part +0.0 or -0.0 in its bits
    (maus_real_values_flagged).  Needs neither a context nor a device."""
    v = _c128(np.ravel(np.asarray(values, dtype=np.complex128)))
    r = load_library().maus_real_values_flagged(_ptr(v), int(v.shape[0]))
    if r < 0:
        raise MausHipError("maus_real_values_flagged: bad arguments")
    return bool(r)


def spmm_plan(method, fill_cap_percent, rows, nnz, padded) -> int:
    """The kernel of an operand with `rows` rows, nnz entries and `padded` sliced-ELL slots under (method, fill_cap_percent)
    (maus_spmm_plan): SPMM_KERNEL_ROWS, SPMM_KERNEL_WAVE or SPMM_KERNEL_SELL.  Needs neither a context nor a device."""
    kind = C.c_int()
    if load_library().maus_spmm_plan(int(method), int(fill_cap_percent), int(rows), int(nnz), int(padded), C.byref(kind)) != 0:
        raise MausHipError(f"maus_spmm_plan: bad method, cap or sizes ({method}, {fill_cap_percent}, {rows}, {nnz}, {padded})")
    return int(kind.value)


def comm_unique_id() -> bytes:
    """A fresh RCCL unique id (one rank creates it, every rank passes it to Context.comm_init)."""
    lib = load_library()
    buf = C.create_string_buffer(COMM_ID_BYTES)
    if lib.maus_comm_unique_id(buf) != 0:
        msg = lib.maus_last_error(None)
        raise MausHipError(f"maus_comm_unique_id failed: {msg.decode() if msg else ''}")
    return buf.raw


def mt19937_jump(key: np.ndarray, pos: int, nwords: int):
    """Advance a legacy NumPy MT19937 (key[624], pos) by nwords 32-bit outputs."""
    lib = load_library()
    k = np.ascontiguousarray(key, dtype=np.uint32).copy()
    p = C.c_int32(int(pos))
    rc = lib.maus_mt19937_jump(_ptr(k), C.byref(p), C.c_uint64(int(nwords)))
    if rc != 0:
        raise MausHipError("maus_mt19937_jump failed")
    return k, int(p.value)
