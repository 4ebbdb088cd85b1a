"""ctypes binding of libmomcore.so (include/momcore.h).

There is no CPU fallback: if the HIP library is missing or a call fails, a `MomError` is
raised.  The library is built in-tree (radiativetransfer.jl_amd/libmomcore.so) by
`make -C radiativetransfer.jl_amd/csrc` or `__graft_entry__.build()`.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
# MOM_LIBRARY: another build of the same HIP library (kernel A/B experiments); never a CPU substitute
LIB_PATH = Path(os.environ["MOM_LIBRARY"]) if os.environ.get("MOM_LIBRARY") else PKG_DIR / "libmomcore.so"

c_dp = C.POINTER(C.c_double)
c_ip = C.POINTER(C.c_int)
c_h = C.c_void_p

MOM_OK, MOM_EINVAL, MOM_EHIP, MOM_ESTATE, MOM_ESINGULAR, MOM_EUNSUPPORTED = 0, -1, -2, -3, -4, -5
_CODES = {MOM_EINVAL: "MOM_EINVAL", MOM_EHIP: "MOM_EHIP", MOM_ESTATE: "MOM_ESTATE", MOM_ESINGULAR: "MOM_ESINGULAR",
          MOM_EUNSUPPORTED: "MOM_EUNSUPPORTED"}

# which-codes of mom_upload / mom_download
ADDED = dict(r_pm=0, r_mp=1, t_mm=2, t_pp=3, j0p=4, j0m=5)
COMP = dict(R_mp=6, R_pm=7, T_pp=8, T_mm=9, J0p=10, J0m=11)
SURF = dict(r_pm=12, r_mp=13, t_mm=14, t_pp=15, j0p=16, j0m=17)
# ... of mom_rrs_upload / mom_rrs_download: the codes above for the elastic fields of the RRS layers, these for the 4-D fields
IE_ADDED = dict(ier_pm=18, ier_mp=19, iet_mm=20, iet_pp=21, ieJ0p=22, ieJ0m=23)
IE_COMP = dict(ieR_mp=24, ieR_pm=25, ieT_pp=26, ieT_mm=27, ieJ0p=28, ieJ0m=29)

MOM_OPT_INVERSE, MOM_OPT_FORCE_GENERIC, MOM_OPT_M0_REDUCTION, MOM_OPT_SMALL_WG, MOM_OPT_STAGGER, MOM_OPT_SMALL_N, MOM_OPT_LAYER_SWEEP = 0, 1, 2, 3, 4, 5, 6
MOM_OPT_STRIP_PAD = 7
MOM_OPT_LEAN = 8
MOM_OPT_OVERLAP = 9
MOM_OPT_RRS_KERNELS = 10   # mask: 1 WG pairs, 2 ... for 16 < N <= 32, 4 WG points, 8 tile elemental, 16 / 32 fused elemental always / never
MOM_OPT_DUAL_WORKSPACE_MB = 11   # operator workspace of mom_rt_run_dual (0: 60 % of the free HBM)
MOM_OPT_STRIP2 = 12              # N = 52, 56, 60 on the two-buffer 4-wave image first (1, default), 0 = the 8-wave image only
MOM_OPT_STRIP2_SCHED = 13        # its scheduling, a mask (1, default): 1 = shared unit queue, 2 = asymmetric chain priority (off: measured slower); 0 = neither
MOM_OPT_ZERO_SKIP = 14           # leave out the exact-zero products of the zero-weight trailing streams, a mask (7, default): 1 = quad-block image (blocks), 2 = two-buffer strip image (k-steps), 4 = two-buffer strip image (blocks of four rows of a partly live row tile); 0 = every product
MOM_OPT_LUT_BATCH = 15           # (p, T) nodes per batch of mom_lut_build (0, default: 64); the table does not depend on it
MOM_OPT_SOURCES_ONLY = 16        # 1 (default): a sweep launch of mom_rt_run without an observable moment (the (I,Q) sub-problem's, a full-problem launch from moment 1 on) leaves the composite R-+ and T++ out (two-buffer strip and quad-block images); the two arrays then hold the first layer's r-+, t++; 0 = all four operators
MOM_OPT_ELEMENTAL = 17           # 1 (default): the two-buffer strip and quad-block images build the elemental layer in its table form (stream-pair tables once per scene, branch-free batches of four elements; csrc/mom_elemental_tab.hpp); 0 = elemental_build everywhere; outputs are bit for bit the same

# the absorption model (mom_absorption_set_model, mom_lineshape_xsec): HitranModel.broadening, HitranModel.CEF
BROADENING_VOIGT, BROADENING_DOPPLER, BROADENING_LORENTZ = 0, 1, 2
CEF_HW32SD, CEF_HW32VOIGT = 0, 1
MOM_MIE_FULL_K = 1   # mom_mie_nai2 flag: every radius tile sums l to the global n_max (test access; bitwise the same result)
MOM_PCW_MAX_ORDER, MOM_WIGNER_MAX_TABLE_BYTES = 640, 1 << 30   # mom_mie_pcw: largest N_max; mom_wigner_tables: largest table
MOM_MIE_DUAL_MAX_WEIGHT_ROWS, MOM_MIE_INDEX_ROWS = 3, 2   # mom_mie_nai2_dual: at most 3 weight rows; 2 more output rows (n_r, n_i)
MOM_PCW_MAX_WEIGHT_ROWS, MOM_PCW_INDEX_ROWS = 3, 1   # mom_mie_pcw_dual: at most 3 weight rows; the flag that asks for the (n_r, n_i) rows


class MomError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{_CODES.get(code, code)}: {msg}")
        self.code = code


# every symbol include/momcore.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "mom_create": (C.c_int, [C.POINTER(c_h), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mom_destroy": (C.c_int, [c_h]),
    "mom_last_error": (C.c_char_p, [c_h]),
    "mom_last_global_error": (C.c_char_p, []),
    "mom_sync": (C.c_int, [c_h]),
    "mom_check": (C.c_int, [c_h]),
    "mom_set_streams": (C.c_int, [c_h, c_dp, c_dp, C.c_int, C.c_int, C.c_double, c_dp, c_dp, C.c_int]),
    "mom_elemental": (C.c_int, [c_h, C.c_int, C.c_int, c_dp, c_dp, c_dp, c_dp, c_dp, C.c_int]),
    "mom_doubling": (C.c_int, [c_h, C.c_int, c_dp]),
    "mom_interaction": (C.c_int, [c_h, C.c_int, C.c_int]),
    "mom_copy_added_to_composite": (C.c_int, [c_h]),
    "mom_surface_lambertian": (C.c_int, [c_h, C.c_int, C.c_double, c_dp]),
    "mom_elemental_inelastic_rrs": (C.c_int, [c_h, C.c_int, C.c_int, C.c_int, c_ip] + [c_dp] * 13),
    "mom_rrs_set": (C.c_int, [c_h, C.c_int, c_ip, c_dp, C.c_int]),
    "mom_rrs_set_shard": (C.c_int, [c_h, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mom_rrs_elemental": (C.c_int, [c_h, C.c_int, C.c_int] + [c_dp] * 8),
    "mom_rrs_doubling": (C.c_int, [c_h, C.c_int, c_dp]),
    "mom_rrs_interaction": (C.c_int, [c_h, C.c_int, C.c_int]),
    "mom_rrs_copy_added_to_composite": (C.c_int, [c_h]),
    "mom_rrs_surface_lambertian": (C.c_int, [c_h, C.c_int, C.c_double, c_dp]),
    "mom_rrs_upload": (C.c_int, [c_h, C.c_int, c_dp]),
    "mom_rrs_download": (C.c_int, [c_h, C.c_int, c_dp]),
    "mom_scene_set_rrs": (C.c_int, [c_h, c_dp, c_dp, c_dp]),
    "mom_rt_run_rrs": (C.c_int, [c_h]),
    "mom_get_RT_rrs": (C.c_int, [c_h, c_dp, c_dp, c_dp, c_dp, c_dp]),
    "mom_get_hdr_rrs": (C.c_int, [c_h, c_dp, c_dp, c_dp]),
    "mom_rrs_timers": (C.c_int, [c_h, c_dp, c_ip, C.c_int]),
    "mom_batch_inv": (C.c_int, [c_h, C.c_int, C.c_int, c_dp, c_dp]),
    "mom_batched_mul": (C.c_int, [c_h, C.c_int, C.c_int, c_dp, c_dp, c_dp]),
    "mom_batched_mul_dual": (C.c_int, [c_h, C.c_int, C.c_int, C.c_int, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp]),
    "mom_batch_inv_dual": (C.c_int, [c_h, C.c_int, C.c_int, C.c_int, c_dp, c_dp, c_dp, c_dp]),
    "mom_upload": (C.c_int, [c_h, C.c_int, c_dp]),
    "mom_download": (C.c_int, [c_h, C.c_int, c_dp]),
    "mom_scene_set": (C.c_int, [c_h, C.c_int, C.c_int, C.c_int, c_dp, c_dp, c_dp, c_dp, c_dp, c_ip, c_ip, c_dp,
                                C.c_double, C.c_int, c_ip, c_dp, c_dp]),
    "mom_absorption_begin": (C.c_int, [c_h, C.c_int, c_dp]),
    "mom_absorption_set_lines": (C.c_int, [c_h, C.c_int] + [c_dp] * 8 + [c_ip, C.c_int, C.c_int, c_ip, c_dp, c_dp, c_dp]),
    "mom_voigt_tau_abs_layer": (C.c_int, [c_h, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]),
    "mom_voigt_tau_abs_profile": (C.c_int, [c_h, C.c_int, c_dp, c_dp, C.c_double, C.c_double, c_dp, c_dp]),
    "mom_absorption_get_prefactors": (C.c_int, [c_h, C.c_int, c_dp, c_dp, c_dp, c_dp, c_ip, c_ip]),
    "mom_voigt_tau_abs": (C.c_int, [c_h, C.c_int, C.c_int, c_dp, c_dp, c_dp, c_dp, c_ip, c_ip, C.c_double]),
    "mom_absorption_set": (C.c_int, [c_h, C.c_int, c_dp]),
    "mom_absorption_get": (C.c_int, [c_h, c_dp]),
    "mom_voigt_tau_abs_dual": (C.c_int, [c_h, C.c_int, C.c_int] + [c_dp] * 8 + [c_ip, c_ip, C.c_double]),
    "mom_voigt_tau_abs_profile_dual": (C.c_int, [c_h, C.c_int, c_dp, c_dp, C.c_double, C.c_double, c_dp, c_dp]),
    "mom_absorption_get_partials": (C.c_int, [c_h, c_dp]),
    "mom_absorption_get_prefactor_partials": (C.c_int, [c_h, C.c_int, c_dp, c_dp, c_dp, c_dp]),
    "mom_absorption_set_model": (C.c_int, [c_h, C.c_int, C.c_int]),
    "mom_lineshape_tau_abs": (C.c_int, [c_h, C.c_int, C.c_int] + [c_dp] * 5 + [c_ip, c_ip, C.c_double]),
    "mom_lineshape_tau_abs_dual": (C.c_int, [c_h, C.c_int, C.c_int] + [c_dp] * 10 + [c_ip, c_ip, C.c_double]),
    "mom_absorption_get_gamma_l": (C.c_int, [c_h, C.c_int, c_dp, c_dp]),
    "mom_scene_set_optics": (C.c_int, [c_h, C.c_int, C.c_int, C.c_int, c_dp, C.c_double, c_dp, c_dp, c_dp, c_dp, c_dp,
                                       C.c_double, C.c_int, c_ip, c_dp, c_dp]),
    "mom_scene_set_optics_bands": (C.c_int, [c_h, C.c_int, C.c_int, C.c_int, c_ip, C.c_int, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp,
                                             C.c_double, C.c_int, c_ip, c_dp, c_dp]),
    "mom_scene_set_optics_bands_partials": (C.c_int, [c_h, C.c_int] + [c_dp] * 10),
    "mom_scene_get_layers": (C.c_int, [c_h, c_ip, c_ip, c_dp, c_dp, c_dp, c_dp]),
    "mom_scene_set_surface": (C.c_int, [c_h, C.c_int, C.c_int, c_dp, c_dp]),
    "mom_rt_run": (C.c_int, [c_h]),
    "mom_scene_set_partials": (C.c_int, [c_h, C.c_int] + [c_dp] * 8),
    "mom_scene_set_optics_partials": (C.c_int, [c_h, C.c_int] + [c_dp] * 10),
    "mom_scene_get_partials": (C.c_int, [c_h, c_dp, c_dp, c_dp]),
    "mom_rt_run_dual": (C.c_int, [c_h]),
    "mom_get_RT_partials": (C.c_int, [c_h, c_dp, c_dp]),
    "mom_get_hdr_partials": (C.c_int, [c_h, c_dp, c_dp, c_dp]),
    "mom_rt_run_multisensor": (C.c_int, [c_h, C.c_int, c_ip, c_dp, c_dp]),
    "mom_get_RT": (C.c_int, [c_h, c_dp, c_dp]),
    "mom_get_hdr": (C.c_int, [c_h, c_dp, c_dp, c_dp]),
    "mom_get_RT_device": (C.c_int, [c_h, C.c_void_p, C.c_void_p]),
    "mom_postprocess": (C.c_int, [c_h, C.c_int, C.c_int, c_ip, c_dp, C.c_double, c_dp, c_dp]),
    "mom_comm_unique_id": (C.c_int, [C.c_void_p, C.c_size_t]),
    "mom_comm_init": (C.c_int, [c_h, C.c_int, C.c_int, C.c_void_p]),
    "mom_comm_destroy": (C.c_int, [c_h]),
    "mom_allgather": (C.c_int, [c_h, C.c_void_p, C.c_void_p, C.c_size_t]),
    "mom_rrs_check_padding": (C.c_int, [c_h, C.POINTER(C.c_ulonglong)]),
    "mom_rrs_spectra_count": (C.c_size_t, [c_h, C.c_int]),
    "mom_get_spectra_rrs_device": (C.c_int, [c_h, C.c_int, C.c_void_p]),
    "mom_allgather_rrs_device": (C.c_int, [c_h, C.c_int, C.c_void_p]),
    "mom_allgather_RT_device": (C.c_int, [c_h, C.c_void_p]),
    "mom_allgather_RT": (C.c_int, [c_h, c_dp, c_dp]),
    "mom_timers": (C.c_int, [c_h, c_dp, C.c_int, c_ip]),
    "mom_set_option": (C.c_int, [c_h, C.c_int, C.c_int]),
    "mom_strip2_resumed": (C.c_int, [c_h, c_ip, c_ip]),
    "mom_lut_create": (C.c_int, [c_h, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double,
                                 c_ip]),
    "mom_lut_set_table": (C.c_int, [c_h, C.c_int, c_dp]),
    "mom_lut_build": (C.c_int, [c_h, C.c_int, C.c_double, C.c_double, c_dp]),
    "mom_lut_get_table": (C.c_int, [c_h, C.c_int, c_dp]),
    "mom_lut_get_coefficients": (C.c_int, [c_h, C.c_int, c_dp]),
    "mom_lut_xsec": (C.c_int, [c_h, C.c_int, C.c_int, c_dp, C.c_double, C.c_double, c_dp, c_dp]),
    "mom_lut_tau_abs_profile": (C.c_int, [c_h, C.c_int, C.c_int, c_dp, c_dp, c_dp, c_dp]),
    "mom_lut_tau_abs_profile_dual": (C.c_int, [c_h, C.c_int, C.c_int, c_dp, c_dp, c_dp, c_dp]),
    "mom_lut_destroy": (C.c_int, [c_h, C.c_int]),
    "mom_voigt_xsec": (C.c_int, [C.c_int, C.c_int, c_dp, c_dp, c_dp, c_dp, c_ip, c_ip, C.c_int, c_dp, c_dp]),
    "mom_voigt_xsec_dual": (C.c_int, [C.c_int, C.c_int] + [c_dp] * 8 + [c_ip, c_ip, C.c_int, c_dp, c_dp, c_dp]),
    "mom_lineshape_xsec": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int] + [c_dp] * 5 + [c_ip, c_ip, C.c_int, c_dp, c_dp]),
    "mom_lineshape_xsec_dual": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int] + [c_dp] * 10 + [c_ip, c_ip, C.c_int, c_dp, c_dp, c_dp]),
    "mom_voigt_last_kernel_ms": (C.c_double, []),
    "mom_mie_nai2": (C.c_int, [C.c_int, C.c_int, c_dp, C.c_int, c_dp, C.c_double, C.c_double, C.c_double, C.c_int, c_dp, C.c_int, c_dp,
                               c_dp, C.c_int, c_dp, c_dp, c_dp, c_dp, C.c_int, c_dp, c_dp, c_dp, c_dp]),
    "mom_mie_coefficients": (C.c_int, [C.c_int, C.c_int, c_dp, C.c_double, C.c_double, C.c_int, c_dp, c_dp, c_dp, c_dp]),
    "mom_mie_nai2_dual": (C.c_int, [C.c_int, C.c_int, c_dp, C.c_int, c_dp, C.c_double, C.c_double, C.c_double, C.c_int, c_dp, C.c_int,
                                    c_dp, c_dp, C.c_int, c_dp, c_dp, c_dp, c_dp, C.c_int, c_dp, c_dp, c_dp, c_dp]),
    "mom_mie_coefficients_dual": (C.c_int, [C.c_int, C.c_int, c_dp, C.c_double, C.c_double, C.c_int] + [c_dp] * 8),
    "mom_mie_tables": (C.c_int, [C.c_int, C.c_int, c_dp, C.c_int, C.c_int] + [c_dp] * 6),
    "mom_mie_nai2_spectral": (C.c_int, [C.c_int, C.c_int, c_dp, C.c_int, c_dp, C.c_int, c_dp, c_dp, c_dp, C.c_int, c_dp, c_dp, C.c_int,
                                        C.c_int, C.c_int, C.c_int, c_dp, c_dp, c_dp, c_dp]),
    "mom_mie_nai2_spectral_dual": (C.c_int, [C.c_int, C.c_int, c_dp, C.c_int, c_dp, C.c_int, c_dp, c_dp, c_dp, C.c_int, c_dp, c_dp,
                                             C.c_int, C.c_int, C.c_int, C.c_int, c_dp, c_dp, c_dp, c_dp]),
    "mom_mie_pcw": (C.c_int, [C.c_int, C.c_int, c_dp, c_dp, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, c_dp, c_dp, c_dp]),
    "mom_wigner_tables": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, c_dp, c_dp]),
    "mom_pcw_pair_averages": (C.c_int, [C.c_int, C.c_int, c_dp, c_dp, C.c_double, C.c_double, C.c_double, C.c_int] + [c_dp] * 8),
    "mom_mie_pcw_dual": (C.c_int, [C.c_int, C.c_int, c_dp, C.c_int, c_dp, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, c_dp, c_dp,
                                   c_dp]),
    "mom_pcw_pair_averages_dual": (C.c_int, [C.c_int, C.c_int, c_dp, C.c_int, c_dp, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                                             c_dp]),
    "mom_z_moments": (C.c_int, [C.c_int, C.c_int, C.c_int, c_dp, C.c_int, C.c_int, c_ip, c_dp, C.c_int, C.c_int, C.c_int, c_dp, c_dp, c_dp]),
    "mom_scene_stage_greeks": (C.c_int, [c_h, C.c_int, C.c_int, C.c_int, c_ip, c_dp, C.c_int]),
    "mom_scene_stage_greek_partials": (C.c_int, [c_h, C.c_int, C.c_int, c_ip, c_ip, C.c_int, c_ip, c_dp]),
    "mom_scene_get_bases": (C.c_int, [c_h, C.c_int, c_ip, c_ip, c_dp, c_dp]),
    "mom_truncate_phase": (C.c_int, [C.c_int, C.c_int, c_dp, c_dp, C.c_int, C.c_int, C.c_int, C.c_int, c_dp, c_dp, c_dp, c_ip, c_dp]),
}

_lib = None


def load():
    """dlopen libmomcore.so and bind every declared symbol.  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise MomError(MOM_EHIP, f"{LIB_PATH} not found - build it with `make -C {PKG_DIR / 'csrc'}` "
                                 "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def dp(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_dp)


def ip(a: np.ndarray):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_ip)


class Handle:
    """RAII wrapper of mom_t*.  One handle <-> one GPU <-> one stream."""

    def __init__(self, N: int, nStokes: int, S: int, max_m: int = 1, device: int = 0, dtype: int = 0):
        """dtype 0 = Float64 (everything), 1 = Float32 (scene-level path, operator-level API, batched operators)."""
        self.lib = load()
        self.N, self.nS, self.S, self.M = int(N), int(nStokes), int(S), int(max_m)
        self._h = c_h()
        rc = self.lib.mom_create(C.byref(self._h), device, self.N, self.nS, self.S, self.M, int(dtype))
        if rc != MOM_OK:
            msg = self.lib.mom_last_global_error().decode()
            if self._h:
                self.lib.mom_destroy(self._h)
                self._h = c_h()
            raise MomError(rc, msg)

    def check(self, rc):
        if rc != MOM_OK:
            raise MomError(rc, self.lib.mom_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self.lib.mom_destroy(self._h)
            self._h = c_h()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- thin 1:1 wrappers ---------------------------------------------------------------
    def set_option(self, option, value):
        self.check(self.lib.mom_set_option(self._h, option, value))

    def sync(self):
        self.check(self.lib.mom_sync(self._h))

    def check_async(self):
        self.check(self.lib.mom_check(self._h))

    def set_streams(self, qp_muN, wt_muN, imu0_1based, mu0, I0, D, strict=True):
        qp, wt, I0, D = f64(qp_muN), f64(wt_muN), f64(I0), f64(D)
        self.check(self.lib.mom_set_streams(self._h, dp(qp), dp(wt), len(qp), int(imu0_1based), float(mu0), dp(I0),
                                            dp(D), 1 if strict else 0))

    def elemental(self, m, nd, tau_sum, dtau, varpi, Zpp, Zmp, z_batch):
        a = [f64(x) for x in (tau_sum, dtau, varpi, Zpp, Zmp)]
        self.check(self.lib.mom_elemental(self._h, int(m), int(nd), *[dp(x) for x in a], int(z_batch)))

    def doubling(self, nd, expk):
        e = f64(expk).copy()
        self.check(self.lib.mom_doubling(self._h, int(nd), dp(e)))
        return e

    def interaction(self, iface, with_surface_layer=False):
        self.check(self.lib.mom_interaction(self._h, int(iface), 1 if with_surface_layer else 0))

    def copy_added_to_composite(self):
        self.check(self.lib.mom_copy_added_to_composite(self._h))

    def surface_lambertian(self, m, albedo, tau_tot):
        t = f64(tau_tot)
        self.check(self.lib.mom_surface_lambertian(self._h, int(m), float(albedo), dp(t)))

    def upload(self, which, src):
        s = f64(src).reshape(-1)
        self.check(self.lib.mom_upload(self._h, int(which), dp(s)))

    def download(self, which):
        k = which % 6
        out = np.empty((self.N * self.N if k < 4 else self.N) * self.S)
        self.check(self.lib.mom_download(self._h, int(which), dp(out)))
        return out

    def elemental_inelastic_rrs(self, m, ndoubl, i_l1l0, varpi_l1l0, fscatt, tau_sum, dtau, varpi, Zpp, Zmp):
        """elemental_inelastic!(::RRS) (elemental_inelastic.jl:23-91).  Z*: ABI [N,N] flat; returns the six arrays in ABI
        order: ier_mp, iet_pp, ier_pm, iet_mm [N,N,S,nRaman] and ieJ0p, ieJ0m [N,S,nRaman] (flat, column-major)."""
        il = i32(i_l1l0)
        nR = len(il)
        v = [f64(x).reshape(-1) for x in (varpi_l1l0, fscatt, tau_sum, dtau, varpi, Zpp, Zmp)]
        big, vec = self.N * self.N * self.S * nR, self.N * self.S * nR
        out = [np.empty(big) for _ in range(4)] + [np.empty(vec) for _ in range(2)]
        self.check(self.lib.mom_elemental_inelastic_rrs(self._h, int(m), int(ndoubl), nR, ip(il), *[dp(x) for x in v],
                                                        *[dp(x) for x in out]))
        return out

    # -- rotational-Raman path (RS_type::RRS) -------------------------------------------------------
    def rrs_set(self, i_l1l0, varpi_l1l0, rrs_strict_reference=True):
        """The RRS fields the path reads (src/Inelastic/types.jl:13-33); allocates AddedLayerRS / CompositeLayerRS."""
        il, vp = i32(i_l1l0), f64(varpi_l1l0)
        assert il.size == vp.size
        self.nRaman = int(il.size)
        self.check(self.lib.mom_rrs_set(self._h, self.nRaman, ip(il), dp(vp), 1 if rrs_strict_reference else 0))

    def rrs_set_shard(self, nSpec_global, n_glob0, n1_lo, n1_hi):
        """The handle's points are the window [n_glob0, n_glob0 + S) of a global axis; this rank owns [n1_lo, n1_hi)."""
        self.check(self.lib.mom_rrs_set_shard(self._h, int(nSpec_global), int(n_glob0), int(n1_lo), int(n1_hi)))

    def rrs_elemental(self, m, nd, tau_sum, dtau, varpi, Zpp, Zmp, fscatt, Zpp_l1l0, Zmp_l1l0):
        a = [f64(x).reshape(-1) for x in (tau_sum, dtau, varpi, Zpp, Zmp, fscatt, Zpp_l1l0, Zmp_l1l0)]
        self.check(self.lib.mom_rrs_elemental(self._h, int(m), int(nd), *[dp(x) for x in a]))

    def rrs_doubling(self, nd, expk):
        e = f64(expk).copy()
        self.check(self.lib.mom_rrs_doubling(self._h, int(nd), dp(e)))
        return e

    def rrs_interaction(self, iface, with_surface_layer=False):
        self.check(self.lib.mom_rrs_interaction(self._h, int(iface), 1 if with_surface_layer else 0))

    def rrs_copy_added_to_composite(self):
        self.check(self.lib.mom_rrs_copy_added_to_composite(self._h))

    def rrs_surface_lambertian(self, m, albedo, tau_tot):
        t = f64(tau_tot)
        self.check(self.lib.mom_rrs_surface_lambertian(self._h, int(m), float(albedo), dp(t)))

    def rrs_upload(self, which, src):
        s = f64(src).reshape(-1)
        assert s.size == self._rrs_count(which)
        self.check(self.lib.mom_rrs_upload(self._h, int(which), dp(s)))

    def _rrs_count(self, which):
        return (self.N * self.N if which % 6 < 4 else self.N) * self.S * (self.nRaman if which >= 18 else 1)

    def rrs_download(self, which):
        out = np.empty(self._rrs_count(which))
        self.check(self.lib.mom_rrs_download(self._h, int(which), dp(out)))
        return out

    def scene_set_rrs(self, fscatt, Zpp_l1l0, Zmp_l1l0):
        a = [None if x is None else f64(x).reshape(-1) for x in (fscatt, Zpp_l1l0, Zmp_l1l0)]   # Z None: the staged Raman set
        self.check(self.lib.mom_scene_set_rrs(self._h, *[None if x is None else dp(x) for x in a]))

    def rt_run_rrs(self):
        self.check(self.lib.mom_rt_run_rrs(self._h))

    def get_RT_rrs(self):
        """(R_SFI, T_SFI, ieR_SFI, ieT_SFI), each [nVza, nStokes, S], and the GPU time of the run in ms."""
        out = [np.empty(self.nVza * self.nS * self.S) for _ in range(4)]
        ms = np.zeros(1)
        self.check(self.lib.mom_get_RT_rrs(self._h, *[dp(x) for x in out], dp(ms)))
        sh = (self.S, self.nS, self.nVza)
        return tuple(np.transpose(x.reshape(sh), (2, 1, 0)).copy() for x in out) + (float(ms[0]),)

    def get_hdr_rrs(self):
        """hdr [nVza, nStokes, S], bhr_uw, bhr_dw [nStokes, S] of the last rt_run_rrs."""
        n = self.nVza * self.nS * self.S
        H, up, dw = np.empty(n), np.empty(self.nS * self.S), np.empty(self.nS * self.S)
        self.check(self.lib.mom_get_hdr_rrs(self._h, dp(H), dp(up), dp(dw)))
        return (np.transpose(H.reshape(self.S, self.nS, self.nVza), (2, 1, 0)).copy(), up.reshape(self.S, self.nS).T.copy(),
                dw.reshape(self.S, self.nS).T.copy())

    def rrs_check_padding(self) -> int:
        """Nonzero entries in the zero padding of the RRS layer arrays (0 = the whole-tile stores kept the invariant)."""
        v = C.c_ulonglong(0)
        self.check(self.lib.mom_rrs_check_padding(self._h, C.byref(v)))
        return int(v.value)

    def rrs_spectra_count(self, per: int) -> int:
        return int(self.lib.mom_rrs_spectra_count(self._h, int(per)))

    def get_spectra_rrs_device(self, per: int, d_local_ptr: int):
        """Owned slices of the seven spectra packed into a device buffer of rrs_spectra_count(per) doubles (asynchronous)."""
        self.check(self.lib.mom_get_spectra_rrs_device(self._h, int(per), C.c_void_p(d_local_ptr)))

    def allgather_rrs_device(self, per: int, d_global_ptr: int):
        """One RCCL all-gather of every rank's packed owned spectra into [nranks][rrs_spectra_count(per)] (asynchronous)."""
        self.check(self.lib.mom_allgather_rrs_device(self._h, int(per), C.c_void_p(d_global_ptr)))

    def rrs_timers(self):
        """{kernel: (ms, launches)} of the last rt_run_rrs (HIP events on the library's stream)."""
        ms, nl = np.zeros(4), np.zeros(4, dtype=np.int32)
        self.check(self.lib.mom_rrs_timers(self._h, dp(ms), ip(nl), 4))
        return {k: (float(ms[i]), int(nl[i])) for i, k in enumerate(("dbl_pair", "int_pair", "ie_elemental", "total"))}

    def batch_inv(self, n, batch, A):
        A = f64(A).reshape(-1)
        X = np.empty_like(A)
        self.check(self.lib.mom_batch_inv(self._h, n, batch, dp(A), dp(X)))
        return X

    def batched_mul(self, n, batch, A, B):
        A, B = f64(A).reshape(-1), f64(B).reshape(-1)
        Cm = np.empty_like(A)
        self.check(self.lib.mom_batched_mul(self._h, n, batch, dp(A), dp(B), dp(Cm)))
        return Cm

    def batch_inv_dual(self, n, batch, P, A, dA):
        """Dual batch_inv! (gpu_batched.jl:129-150): flat ABI arrays, values n*n*batch, partials n*n*batch*P."""
        A, dA = f64(A).reshape(-1), f64(dA).reshape(-1)
        X, dX = np.empty_like(A), np.empty_like(dA)
        self.check(self.lib.mom_batch_inv_dual(self._h, n, batch, P, dp(A), dp(dA), dp(X), dp(dX)))
        return X, dX

    def batched_mul_dual(self, n, batch, P, A, dA, B, dB):
        """Dual batched_mul (gpu_batched.jl:100-110)."""
        A, dA, B, dB = (f64(x).reshape(-1) for x in (A, dA, B, dB))
        Cm, dC = np.empty_like(A), np.empty_like(dA)
        self.check(self.lib.mom_batched_mul_dual(self._h, n, batch, P, dp(A), dp(dA), dp(B), dp(dB), dp(Cm), dp(dC)))
        return Cm, dC

    def scene_set(self, Nz, K, M, tau, varpi, zw, Zpp, Zmp, nd, iface, tau_sum, albedo, node, cos_mphi, sin_mphi):
        d = [None if x is None else f64(x).reshape(-1) for x in (tau, varpi, zw, Zpp, Zmp)]   # Zpp, Zmp None: the staged bases
        nd, iface, node = i32(nd), i32(iface), i32(node)
        ts, cm, sm = f64(tau_sum).reshape(-1), f64(cos_mphi).reshape(-1), f64(sin_mphi).reshape(-1)
        self.nVza = len(node)
        self._Nz, self._K = int(Nz), int(K)
        self.check(self.lib.mom_scene_set(self._h, int(Nz), int(K), int(M), *[None if x is None else dp(x) for x in d], ip(nd), ip(iface),
                                          dp(ts), float(albedo), len(node), ip(node), dp(cm), dp(sm)))

    # -- device-side layer optics --------------------------------------------------------------
    def absorption_begin(self, Nz, grid=None):
        g = f64(grid) if grid is not None else None
        assert g is None or g.size == self.S
        self._absNz = int(Nz)
        self.check(self.lib.mom_absorption_begin(self._h, int(Nz), dp(g) if g is not None else None))

    def absorption_set(self, tau_abs):
        """tau_abs: [S, Nz] numpy (reference layout)."""
        t = np.ascontiguousarray(np.asarray(tau_abs, dtype=np.float64).T).reshape(-1)  # column-major [S, Nz]
        self._absNz = int(np.asarray(tau_abs).shape[1])
        self.check(self.lib.mom_absorption_set(self._h, self._absNz, dp(t)))

    def absorption_get(self):
        out = np.empty(self.S * self._absNz)
        self.check(self.lib.mom_absorption_get(self._h, dp(out)))
        return out.reshape(self._absNz, self.S).T.copy()

    def voigt_tau_abs(self, iz_1based, nu, gamma_d, y, S, ind_start, ind_stop, factor):
        a = [f64(x) for x in (nu, gamma_d, y, S)]
        i0, i1 = i32(ind_start), i32(ind_stop)
        self.check(self.lib.mom_voigt_tau_abs(self._h, int(iz_1based), len(a[0]), *[dp(x) for x in a], ip(i0), ip(i1),
                                              float(factor)))

    def absorption_set_lines(self, cols, sqrt_w, iso_index, nT, tips_T, tips_Q, tips_z):
        """cols: the eight per-line arrays nu0, S0, gamma_air, gamma_self, E_lower, n_air, delta_air (+ sqrt_w appended here);
        tips_*: [nIso, nTmax] numpy."""
        a = [f64(x) for x in cols] + [f64(sqrt_w)]
        ii, nT = i32(iso_index), i32(nT)
        tt, tq, tz = (f64(x) for x in (tips_T, tips_Q, tips_z))
        nIso, nTmax = (tt.shape if tt.ndim == 2 else (0, 0))
        self._nLines = len(a[0])
        self.check(self.lib.mom_absorption_set_lines(self._h, self._nLines, *[dp(x) for x in a], ip(ii), int(nIso), int(nTmax),
                                                     ip(nT), dp(tt.reshape(-1)), dp(tq.reshape(-1)), dp(tz.reshape(-1))))

    def voigt_tau_abs_layer(self, iz_1based, p, T, vmr, wing_cutoff, factor):
        self.check(self.lib.mom_voigt_tau_abs_layer(self._h, int(iz_1based), float(p), float(T), float(vmr), float(wing_cutoff),
                                                    float(factor)))

    def voigt_tau_abs_profile(self, p, T, vmr, wing_cutoff, factor) -> float:
        """All layers 1..len(p) in two launches (mom_voigt_tau_abs_profile); returns the GPU time of the two kernels in ms."""
        p, T, f = f64(p), f64(T), f64(factor)
        assert p.size == T.size == f.size
        ms = np.zeros(1)
        self.check(self.lib.mom_voigt_tau_abs_profile(self._h, int(p.size), dp(p), dp(T), float(vmr), float(wing_cutoff), dp(f), dp(ms)))
        return float(ms[0])

    def absorption_get_prefactors(self, n=None):
        n = self._nLines if n is None else int(n)
        d = [np.empty(n) for _ in range(4)]
        i0, i1 = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        self.check(self.lib.mom_absorption_get_prefactors(self._h, n, *[dp(x) for x in d], ip(i0), ip(i1)))
        return d + [i0, i1]

    # -- the Dual run of the absorption path: partials with respect to (p, T) of each layer ------------------
    def voigt_tau_abs_dual(self, iz_1based, nu, gamma_d, y, S, dnu, dgamma_d, dy, dS, ind_start, ind_stop, factor):
        """mom_voigt_tau_abs_dual: the partials of the four prefactors as [nLines, 2] numpy (column 0: pressure, 1:
        temperature) or None (zeros)."""
        a = [f64(x) for x in (nu, gamma_d, y, S)]
        d = [_partials(x, len(a[0])) for x in (dnu, dgamma_d, dy, dS)]
        i0, i1 = i32(ind_start), i32(ind_stop)
        self.check(self.lib.mom_voigt_tau_abs_dual(self._h, int(iz_1based), len(a[0]), *[dp(x) for x in a],
                                                   *[None if x is None else dp(x) for x in d], ip(i0), ip(i1), float(factor)))

    def voigt_tau_abs_profile_dual(self, p, T, vmr, wing_cutoff, factor) -> float:
        """voigt_tau_abs_profile that also adds the partials into the resident dtau_abs table; returns the GPU time in ms."""
        p, T, f = f64(p), f64(T), f64(factor)
        assert p.size == T.size == f.size
        ms = np.zeros(1)
        self.check(self.lib.mom_voigt_tau_abs_profile_dual(self._h, int(p.size), dp(p), dp(T), float(vmr), float(wing_cutoff), dp(f),
                                                           dp(ms)))
        return float(ms[0])

    # -- the absorption model (HitranModel.broadening x HitranModel.CEF) ------------------------------------
    def absorption_set_model(self, broadening=BROADENING_VOIGT, cef=CEF_HW32SD):
        """mom_absorption_set_model: the model of every later absorption call on the handle (codes BROADENING_*, CEF_*)."""
        self.check(self.lib.mom_absorption_set_model(self._h, int(broadening), int(cef)))

    def lineshape_tau_abs(self, iz_1based, nu, gamma_d, gamma_l, y, S, ind_start, ind_stop, factor):
        """mom_lineshape_tau_abs: voigt_tau_abs for the handle's model; an array its broadening does not read may be None."""
        a = [None if x is None else f64(x) for x in (nu, gamma_d, gamma_l, y, S)]
        i0, i1 = i32(ind_start), i32(ind_stop)
        self.check(self.lib.mom_lineshape_tau_abs(self._h, int(iz_1based), len(a[0]), *[None if x is None else dp(x) for x in a],
                                                  ip(i0), ip(i1), float(factor)))

    def lineshape_tau_abs_dual(self, iz_1based, nu, gamma_d, gamma_l, y, S, dnu, dgamma_d, dgamma_l, dy, dS, ind_start, ind_stop,
                               factor):
        """mom_lineshape_tau_abs_dual: the partials of the five prefactors as [nLines, 2] numpy or None (zeros)."""
        a = [None if x is None else f64(x) for x in (nu, gamma_d, gamma_l, y, S)]
        d = [_partials(x, len(a[0])) for x in (dnu, dgamma_d, dgamma_l, dy, dS)]
        i0, i1 = i32(ind_start), i32(ind_stop)
        self.check(self.lib.mom_lineshape_tau_abs_dual(self._h, int(iz_1based), len(a[0]), *[None if x is None else dp(x) for x in a],
                                                       *[None if x is None else dp(x) for x in d], ip(i0), ip(i1), float(factor)))

    def absorption_get_gamma_l(self, n=None, partials=False):
        """gamma_l [n] of the last device-prefactor call; partials=True: (gamma_l, dgamma_l [n, 2]) of the last Dual call."""
        n = self._nLines if n is None else int(n)
        g, d = np.empty(n), (np.empty(2 * n) if partials else None)
        self.check(self.lib.mom_absorption_get_gamma_l(self._h, n, dp(g), dp(d) if partials else None))
        return (g, d.reshape(2, n).T.copy()) if partials else g

    def absorption_get_partials(self):
        """dtau_abs as numpy [2, S, Nz]: [0] with respect to the layer's pressure, [1] to its temperature."""
        out = np.empty(2 * self.S * self._absNz)
        self.check(self.lib.mom_absorption_get_partials(self._h, dp(out)))
        return np.transpose(out.reshape(2, self._absNz, self.S), (0, 2, 1)).copy()

    def absorption_get_prefactor_partials(self, n=None):
        """dnu, dgamma_d, dy, dS of the last Dual call, each [n, 2] numpy."""
        n = self._nLines if n is None else int(n)
        d = [np.empty(2 * n) for _ in range(4)]
        self.check(self.lib.mom_absorption_get_prefactor_partials(self._h, n, *[dp(x) for x in d]))
        return [x.reshape(2, n).T.copy() for x in d]

    # -- the InterpolationModel: sigma(nu, p, T) tables resident on the device (mom_lut_*) ----------------------
    def lut_create(self, nu_range, p_range, t_range) -> int:
        """mom_lut_create: each range is (first, step, length); returns the table's id."""
        (n0, s0, l0), (n1, s1, l1), (n2, s2, l2) = nu_range, p_range, t_range
        lut = C.c_int(-1)
        self.check(self.lib.mom_lut_create(self._h, int(l0), float(n0), float(s0), int(l1), float(n1), float(s1), int(l2), float(n2),
                                           float(s2), C.byref(lut)))
        self._lut_shape = getattr(self, "_lut_shape", {})
        self._lut_shape[lut.value] = (int(l0), int(l1), int(l2))
        return lut.value

    def _lut_dims(self, lut):
        return getattr(self, "_lut_shape", {}).get(int(lut), (1, 1, 1))   # an unknown id: the library reports it

    def lut_set_table(self, lut, sigma):
        """sigma: numpy [nNu, nP, nT] (the reference's cs_matrix); uploaded nu fastest and prefiltered on the device."""
        s = np.asarray(sigma, dtype=np.float64)
        assert s.shape == self._lut_dims(lut), (s.shape, self._lut_dims(lut))
        flat = np.ascontiguousarray(s.transpose(2, 1, 0)).reshape(-1)
        self.check(self.lib.mom_lut_set_table(self._h, int(lut), dp(flat)))

    def lut_build(self, lut, vmr=0.0, wing_cutoff=40.0):
        """mom_lut_build from the resident line table; returns (fill ms, prefilter ms) of the GPU."""
        ms = np.zeros(2)
        self.check(self.lib.mom_lut_build(self._h, int(lut), float(vmr), float(wing_cutoff), dp(ms)))
        return float(ms[0]), float(ms[1])

    def lut_get_table(self, lut):
        n = self._lut_dims(lut)
        out = np.empty(n[0] * n[1] * n[2])
        self.check(self.lib.mom_lut_get_table(self._h, int(lut), dp(out)))
        return out.reshape(n[2], n[1], n[0]).transpose(2, 1, 0).copy()

    def lut_get_coefficients(self, lut):
        """The padded cubic B-spline coefficients as numpy [nNu + 2, nP + 2, nT + 2]."""
        n = [k + 2 for k in self._lut_dims(lut)]
        out = np.empty(n[0] * n[1] * n[2])
        self.check(self.lib.mom_lut_get_coefficients(self._h, int(lut), dp(out)))
        return out.reshape(n[2], n[1], n[0]).transpose(2, 1, 0).copy()

    def lut_xsec(self, lut, nu, p, T, jacobian=False):
        """mom_lut_xsec: sigma [n], or with jacobian=True (sigma, J [n, 2]) with column 0 = d/dp and 1 = d/dT."""
        nu = f64(nu).reshape(-1)
        sigma, J = np.empty(nu.size), (np.empty(2 * nu.size) if jacobian else None)
        self.check(self.lib.mom_lut_xsec(self._h, int(lut), int(nu.size), dp(nu), float(p), float(T), dp(sigma),
                                         dp(J) if jacobian else None))
        return (sigma, J.reshape(2, nu.size).T.copy()) if jacobian else sigma

    def lut_tau_abs_profile(self, lut, p, T, factor, dual=False) -> float:
        """mom_lut_tau_abs_profile(_dual) for layers 1..len(p); returns the GPU time of the launch in ms."""
        p, T, f = f64(p), f64(T), f64(factor)
        assert p.size == T.size == f.size
        ms = np.zeros(1)
        fn = self.lib.mom_lut_tau_abs_profile_dual if dual else self.lib.mom_lut_tau_abs_profile
        self.check(fn(self._h, int(lut), int(p.size), dp(p), dp(T), dp(f), dp(ms)))
        return float(ms[0])

    def lut_destroy(self, lut):
        self.check(self.lib.mom_lut_destroy(self._h, int(lut)))
        getattr(self, "_lut_shape", {}).pop(int(lut), None)

    def scene_set_optics(self, Nz, M, tau_rayl, varpi_rayl, tau_aer, omega_aer, ft_aer, Zpp, Zmp, albedo, node, cos_mphi,
                         sin_mphi):
        """tau_rayl [S, Nz], tau_aer [nAer, Nz] numpy (reference layouts); Zpp/Zmp already in ABI order."""
        tr = np.ascontiguousarray(np.asarray(tau_rayl, dtype=np.float64).T).reshape(-1)
        ta = np.asarray(tau_aer, dtype=np.float64)
        nAer = ta.shape[0] if ta.size else 0
        taf = np.ascontiguousarray(ta.T).reshape(-1) if nAer else np.zeros(1)  # [nAer, Nz] column-major
        om, ft = (f64(omega_aer), f64(ft_aer)) if nAer else (np.zeros(1), np.zeros(1))
        zp, zm = (None if z is None else dp(f64(z).reshape(-1)) for z in (Zpp, Zmp))   # None: the staged bases
        node = i32(node)
        cm, sm = f64(cos_mphi).reshape(-1), f64(sin_mphi).reshape(-1)
        self.nVza = len(node)
        self._Nz, self._K = int(Nz), 1 + nAer
        self.check(self.lib.mom_scene_set_optics(self._h, int(Nz), nAer, int(M), dp(tr), float(varpi_rayl), dp(taf), dp(om),
                                                 dp(ft), zp, zm, float(albedo), len(node), ip(node), dp(cm), dp(sm)))

    def scene_set_optics_bands(self, Nz, M, band_start, tau_rayl, varpi_rayl, tau_aer, omega_aer, ft_aer, Zpp, Zmp, albedo, node,
                               cos_mphi, sin_mphi):
        """mom_scene_set_optics_bands: band_start [nBand + 1], tau_rayl [S, Nz], varpi_rayl [nBand], tau_aer [nBand, nAer, Nz],
        omega_aer / ft_aer [nBand, nAer] numpy (reference layouts); Zpp/Zmp already in ABI order, K = 1 + nAer nBand bases."""
        bs = i32(np.asarray(band_start).reshape(-1))
        nBand = bs.size - 1
        tr = np.ascontiguousarray(np.asarray(tau_rayl, dtype=np.float64).T).reshape(-1)
        ta = np.asarray(tau_aer, dtype=np.float64)
        nAer = ta.shape[1] if ta.ndim == 3 and ta.size else 0
        vr = f64(varpi_rayl).reshape(-1)
        taf = np.ascontiguousarray(ta.transpose(0, 2, 1)).reshape(-1) if nAer else np.zeros(1)  # [nAer, Nz, nBand], iAer fastest
        om, ft = (f64(omega_aer).reshape(-1), f64(ft_aer).reshape(-1)) if nAer else (np.zeros(1), np.zeros(1))
        assert vr.size == max(nBand, 1) and (not nAer or (ta.shape[0] == nBand and om.size == ft.size == nBand * nAer))
        zp, zm = (None if z is None else dp(f64(z).reshape(-1)) for z in (Zpp, Zmp))   # None: the staged bases
        node = i32(node)
        cm, sm = f64(cos_mphi).reshape(-1), f64(sin_mphi).reshape(-1)
        self.nVza = len(node)
        self._Nz, self._K = int(Nz), 1 + nAer * nBand
        self.check(self.lib.mom_scene_set_optics_bands(self._h, int(Nz), nAer, nBand, ip(bs), int(M), dp(tr), dp(vr), dp(taf), dp(om),
                                                       dp(ft), zp, zm, float(albedo), len(node), ip(node), dp(cm), dp(sm)))

    # -- scenes from Greek coefficients: the Z bases formed in the handle's memory ------------------------
    def scene_stage_greeks(self, greeks, M, which=0):
        """mom_scene_stage_greeks: `greeks` as in z_moments (each set the six rows α, β, γ, δ, ϵ, ζ of its own length).  which = 0: the
        bases of the next scene setter called with Zpp = Zmp = None; 1: the one Raman set of the next scene_set_rrs."""
        nG, l_pad, l_max, greek = pack_greeks(greeks, "scene_stage_greeks")
        self.check(self.lib.mom_scene_stage_greeks(self._h, int(which), nG, l_pad, ip(l_max), dp(greek), int(M)))

    def scene_stage_greek_partials(self, P, pairs):
        """mom_scene_stage_greek_partials: `pairs` is a sequence of ((basis k, partial p), derivative Greek set); the next partial
        setter called with dZpp = dZmp = None and this P takes them."""
        nD, l_pad, l_max, greek = pack_greeks([g for _, g in pairs], "scene_stage_greek_partials")
        basis, partial = i32([kp[0] for kp, _ in pairs]), i32([kp[1] for kp, _ in pairs])
        self.check(self.lib.mom_scene_stage_greek_partials(self._h, int(P), nD, ip(basis), ip(partial), l_pad, ip(l_max), dp(greek)))

    def scene_get_bases(self, which=0):
        """mom_scene_get_bases: (edge, Zpp, Zmp) as the kernels read them, C arrays [blocks, edge(j), edge(i)] -- which = 0 the bases
        (blocks = M K, k fastest), 1 the (I,Q) sub-problem's (blocks = K; edge 0 and empty arrays when the scene is not reduced), 2 the
        resident dZ (blocks = P M K), 3 the Raman set (blocks = M)."""
        e, b = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        self.check(self.lib.mom_scene_get_bases(self._h, int(which), ip(e), ip(b), None, None))
        edge, blocks = int(e[0]), int(b[0])
        Zpp, Zmp = np.empty((blocks, edge, edge)), np.empty((blocks, edge, edge))
        if Zpp.size:
            self.check(self.lib.mom_scene_get_bases(self._h, int(which), ip(e), ip(b), dp(Zpp), dp(Zmp)))
        return edge, Zpp, Zmp

    def scene_get_layers(self, Nz, K, arrays=True):
        nd, iface = np.zeros(Nz, dtype=np.int32), np.zeros(Nz, dtype=np.int32)
        S = self.S
        bufs = [np.empty(S * Nz), np.empty(S * Nz), np.empty(K * S * Nz), np.empty(S * (Nz + 1))] if arrays else [None] * 4
        self.check(self.lib.mom_scene_get_layers(self._h, ip(nd), ip(iface), *[dp(b) if b is not None else None for b in bufs]))
        return (nd, iface) + tuple(bufs)

    def scene_set_surface(self, kind, M=0, Rsurf=None, albedo_spec=None):
        """Rsurf: already in ABI order ([N, N, M], i fastest); albedo_spec: [S]."""
        r = f64(Rsurf).reshape(-1) if Rsurf is not None else None
        al = f64(albedo_spec).reshape(-1) if albedo_spec is not None else None
        self.check(self.lib.mom_scene_set_surface(self._h, int(kind), int(M), dp(r) if r is not None else None,
                                                  dp(al) if al is not None else None))

    def rt_run(self):
        self.check(self.lib.mom_rt_run(self._h))

    # -- rt_run on ForwardDiff.Dual numbers (mom_dual.hip) ------------------------------------------
    def scene_set_partials(self, P, dtau=None, dvarpi=None, dzw=None, dZpp=None, dZmp=None, dalbedo=None, dRsurf=None,
                           dalbedo_spec=None):
        """Partials of the scene's inputs, flat buffers in ABI order (partial index slowest); None = no dependence."""
        bufs = [None if x is None else f64(x).reshape(-1) for x in (dtau, dvarpi, dzw, dZpp, dZmp, dalbedo, dRsurf, dalbedo_spec)]
        self.dual_P = int(P)
        self.check(self.lib.mom_scene_set_partials(self._h, int(P), *[None if b is None else dp(b) for b in bufs]))

    def scene_set_optics_partials(self, P, w_abs=None, w_rayl=None, dtau_aer=None, domega_aer=None, dft_aer=None, dZpp=None,
                                  dZmp=None, dalbedo=None, dRsurf=None, dalbedo_spec=None):
        """mom_scene_set_optics_partials: the partials of the INGREDIENTS of a scene_set_optics scene, flat buffers in ABI order
        (w_abs [Nz, 3, P], w_rayl [Nz, P], dtau_aer [nAer, Nz, P], domega_aer, dft_aer [nAer, P], partial index slowest; the rest as
        in scene_set_partials); None = no dependence.  The device forms dtau, dvarpi, dzw."""
        bufs = [None if x is None else f64(x).reshape(-1)
                for x in (w_abs, w_rayl, dtau_aer, domega_aer, dft_aer, dZpp, dZmp, dalbedo, dRsurf, dalbedo_spec)]
        self.check(self.lib.mom_scene_set_optics_partials(self._h, int(P), *[None if b is None else dp(b) for b in bufs]))
        self.dual_P = int(P)

    def scene_set_optics_bands_partials(self, P, w_abs=None, w_rayl=None, dtau_aer=None, domega_aer=None, dft_aer=None, dZpp=None,
                                        dZmp=None, dalbedo=None, dRsurf=None, dalbedo_spec=None):
        """mom_scene_set_optics_bands_partials: scene_set_optics_partials for a scene_set_optics_bands scene; the aerosol partials carry
        a band axis (dtau_aer [nAer, Nz, nBand, P], domega_aer, dft_aer [nAer, nBand, P])."""
        bufs = [None if x is None else f64(x).reshape(-1)
                for x in (w_abs, w_rayl, dtau_aer, domega_aer, dft_aer, dZpp, dZmp, dalbedo, dRsurf, dalbedo_spec)]
        self.check(self.lib.mom_scene_set_optics_bands_partials(self._h, int(P), *[None if b is None else dp(b) for b in bufs]))
        self.dual_P = int(P)

    def scene_get_partials(self):
        """The resident partials of the scene as numpy in the reference's shapes: dτ, dϖ [P, nSpec, Nz], dzw [P, K, nSpec, Nz]
        (an absent device buffer reads as zeros)."""
        P, S, Nz, K = getattr(self, "dual_P", 0), self.S, getattr(self, "_Nz", 1), getattr(self, "_K", 1)   # no scene: the library says so
        n = max(P * S * Nz, 1)
        dt, dv, dz = np.empty(n), np.empty(n), np.empty(K * n)
        self.check(self.lib.mom_scene_get_partials(self._h, dp(dt), dp(dv), dp(dz)))
        tr = lambda a: np.transpose(a.reshape(P, Nz, S), (0, 2, 1)).copy()
        return tr(dt), tr(dv), np.transpose(dz.reshape(P, Nz, S, K), (0, 3, 2, 1)).copy()

    def rt_run_dual(self):
        self.check(self.lib.mom_rt_run_dual(self._h))

    def get_RT_partials(self):
        """dR_SFI, dT_SFI as numpy [P, nVza, nStokes, S]."""
        P = self.dual_P
        n = self.nVza * self.nS * self.S * P
        dR, dT = np.empty(n), np.empty(n)
        self.check(self.lib.mom_get_RT_partials(self._h, dp(dR), dp(dT)))
        shp = (P, self.S, self.nS, self.nVza)
        return np.transpose(dR.reshape(shp), (0, 3, 2, 1)).copy(), np.transpose(dT.reshape(shp), (0, 3, 2, 1)).copy()

    def get_hdr_partials(self):
        """dhdr [P, nVza, nStokes, S], dbhr_uw, dbhr_dw [P, nStokes, S]."""
        P = self.dual_P
        n, f = self.nVza * self.nS * self.S * P, self.nS * self.S * P
        dH, up, dw = np.empty(n), np.empty(f), np.empty(f)
        self.check(self.lib.mom_get_hdr_partials(self._h, dp(dH), dp(up), dp(dw)))
        tr = lambda x: np.transpose(x.reshape(P, self.S, self.nS), (0, 2, 1)).copy()
        return np.transpose(dH.reshape(P, self.S, self.nS, self.nVza), (0, 3, 2, 1)).copy(), tr(up), tr(dw)

    def rt_run_multisensor(self, sensor_levels):
        """uwJ, dwJ as numpy [nSensors, nVza, nStokes, S] (the reference's vector of [nVza, nStokes, nSpec] arrays,
        rt_run_multisensor.jl:52-55)."""
        lv = np.ascontiguousarray(sensor_levels, dtype=np.int32)
        n = self.nVza * self.nS * self.S * len(lv)
        uw, dw = np.empty(n), np.empty(n)
        self.check(self.lib.mom_rt_run_multisensor(self._h, len(lv), ip(lv), dp(uw), dp(dw)))
        shp = (len(lv), self.S, self.nS, self.nVza)
        tr = lambda a: np.transpose(a.reshape(shp), (0, 3, 2, 1)).copy()
        return tr(uw), tr(dw)

    def get_RT(self):
        """R_SFI, T_SFI as numpy [nVza, nStokes, S] (reference layout, rt_run.jl:89-90)."""
        n = self.nVza * self.nS * self.S
        R, T = np.empty(n), np.empty(n)
        self.check(self.lib.mom_get_RT(self._h, dp(R), dp(T)))
        shp = (self.S, self.nS, self.nVza)
        return np.transpose(R.reshape(shp), (2, 1, 0)).copy(), np.transpose(T.reshape(shp), (2, 1, 0)).copy()

    def get_hdr(self):
        """hdr [nVza, nStokes, S], bhr_uw, bhr_dw [nStokes, S]."""
        n = self.nVza * self.nS * self.S
        H, up, dw = np.empty(n), np.empty(self.nS * self.S), np.empty(self.nS * self.S)
        self.check(self.lib.mom_get_hdr(self._h, dp(H), dp(up), dp(dw)))
        return (np.transpose(H.reshape(self.S, self.nS, self.nVza), (2, 1, 0)).copy(),
                up.reshape(self.S, self.nS).T.copy(), dw.reshape(self.S, self.nS).T.copy())

    def get_RT_device(self, dR_ptr: int, dT_ptr: int):
        self.check(self.lib.mom_get_RT_device(self._h, C.c_void_p(dR_ptr), C.c_void_p(dT_ptr)))

    def postprocess(self, m, node_1based, vaz_deg, weight, R_SFI, T_SFI):
        """In-place accumulation into R_SFI/T_SFI given as ABI-ordered flat arrays [nVza, nStokes, S] (v fastest)."""
        node, vaz = i32(node_1based), f64(vaz_deg)
        self.check(self.lib.mom_postprocess(self._h, int(m), len(node), ip(node), dp(vaz), float(weight), dp(R_SFI),
                                            dp(T_SFI)))

    # -- multi-GPU (RCCL behind the C ABI) -------------------------------------------------
    def comm_init(self, rank: int, nranks: int, nccl_id: bytes):
        buf = C.create_string_buffer(bytes(nccl_id), COMM_ID_BYTES)
        self.check(self.lib.mom_comm_init(self._h, int(rank), int(nranks), C.cast(buf, C.c_void_p)))
        self.comm_size = int(nranks)

    def comm_destroy(self):
        self.check(self.lib.mom_comm_destroy(self._h))

    def allgather_RT_device(self, d_global_ptr: int):
        self.check(self.lib.mom_allgather_RT_device(self._h, C.c_void_p(d_global_ptr)))

    def allgather_RT(self):
        """R_SFI, T_SFI [nVza, nStokes, nranks*S_loc] on every rank (one RCCL all-gather)."""
        n = self.nVza * self.nS * self.S * self.comm_size
        R, T = np.empty(n), np.empty(n)
        self.check(self.lib.mom_allgather_RT(self._h, dp(R), dp(T)))
        shp = (self.S * self.comm_size, self.nS, self.nVza)
        return np.transpose(R.reshape(shp), (2, 1, 0)).copy(), np.transpose(T.reshape(shp), (2, 1, 0)).copy()

    def strip2_resumed(self):
        """(units of the two-buffer strip image's last launch, units it left to the 8-wave image through the resume table)"""
        u, l = C.c_int(0), C.c_int(0)
        self.check(self.lib.mom_strip2_resumed(self._h, C.byref(u), C.byref(l)))
        return u.value, l.value

    def timers(self):
        ms = np.zeros(8)
        nl = C.c_int(0)
        self.check(self.lib.mom_timers(self._h, dp(ms), 8, C.byref(nl)))
        return dict(layers_ms=ms[0], surface_ms=ms[1], postprocess_ms=ms[2], total_ms=ms[3], layer_launches=nl.value,
                    full_layers_ms=ms[4], reduced_layers_ms=ms[5], full_launches=int(ms[6]), reduced_launches=int(ms[7]))


COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """RCCL unique id (rank 0 calls this and distributes the bytes)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = load().mom_comm_unique_id(C.cast(buf, C.c_void_p), COMM_ID_BYTES)
    if rc != MOM_OK:
        raise MomError(rc, load().mom_last_global_error().decode())
    return buf.raw


def voigt_xsec(nu, gamma_d, y, S, ind_start, ind_stop, grid, device: int = 0):
    lib = load()
    a = [f64(x) for x in (nu, gamma_d, y, S)]
    i0, i1, g = i32(ind_start), i32(ind_stop), f64(grid)
    sigma = np.empty(len(g))
    rc = lib.mom_voigt_xsec(device, len(a[0]), *[dp(x) for x in a], ip(i0), ip(i1), len(g), dp(g), dp(sigma))
    if rc != MOM_OK:
        raise MomError(rc, lib.mom_last_global_error().decode())
    return sigma


def _partials(x, n):
    """[n, 2] numpy -> the ABI's column-major flat array (index j + n k); None stays None (zeros)"""
    if x is None:
        return None
    x = np.asarray(x, dtype=np.float64)
    assert x.shape == (n, 2), f"partials must be [nLines, 2], got {x.shape}"
    return np.ascontiguousarray(x.T).reshape(-1)


def voigt_xsec_dual(nu, gamma_d, y, S, dnu, dgamma_d, dy, dS, ind_start, ind_stop, grid, device: int = 0):
    """mom_voigt_xsec_dual: sigma [nGrid] and dsigma [nGrid, 2] (column 0: d/dp, 1: d/dT).  The partials of the prefactors are
    [nLines, 2] numpy or None (zeros)."""
    lib = load()
    a = [f64(x) for x in (nu, gamma_d, y, S)]
    d = [_partials(x, len(a[0])) for x in (dnu, dgamma_d, dy, dS)]
    i0, i1, g = i32(ind_start), i32(ind_stop), f64(grid)
    sigma, dsigma = np.empty(len(g)), np.empty(2 * len(g))
    rc = lib.mom_voigt_xsec_dual(device, len(a[0]), *[dp(x) for x in a], *[None if x is None else dp(x) for x in d], ip(i0), ip(i1),
                                 len(g), dp(g), dp(sigma), dp(dsigma))
    if rc != MOM_OK:
        raise MomError(rc, lib.mom_last_global_error().decode())
    return sigma, dsigma.reshape(2, len(g)).T.copy()


def lineshape_xsec(broadening, cef, nu, gamma_d, gamma_l, y, S, ind_start, ind_stop, grid, device: int = 0):
    """mom_lineshape_xsec: voigt_xsec for any absorption model (codes BROADENING_*, CEF_*); an array the broadening does not
    read may be None."""
    lib = load()
    a = [None if x is None else f64(x) for x in (nu, gamma_d, gamma_l, y, S)]
    i0, i1, g = i32(ind_start), i32(ind_stop), f64(grid)
    sigma = np.empty(len(g))
    rc = lib.mom_lineshape_xsec(device, int(broadening), int(cef), len(a[0]), *[None if x is None else dp(x) for x in a], ip(i0),
                                ip(i1), len(g), dp(g), dp(sigma))
    if rc != MOM_OK:
        raise MomError(rc, lib.mom_last_global_error().decode())
    return sigma


def lineshape_xsec_dual(broadening, cef, nu, gamma_d, gamma_l, y, S, dnu, dgamma_d, dgamma_l, dy, dS, ind_start, ind_stop, grid,
                        device: int = 0):
    """mom_lineshape_xsec_dual: sigma [nGrid] and dsigma [nGrid, 2]; the partials [nLines, 2] numpy or None (zeros)."""
    lib = load()
    a = [None if x is None else f64(x) for x in (nu, gamma_d, gamma_l, y, S)]
    d = [_partials(x, len(a[0])) for x in (dnu, dgamma_d, dgamma_l, dy, dS)]
    i0, i1, g = i32(ind_start), i32(ind_stop), f64(grid)
    sigma, dsigma = np.empty(len(g)), np.empty(2 * len(g))
    rc = lib.mom_lineshape_xsec_dual(device, int(broadening), int(cef), len(a[0]), *[None if x is None else dp(x) for x in a],
                                     *[None if x is None else dp(x) for x in d], ip(i0), ip(i1), len(g), dp(g), dp(sigma), dp(dsigma))
    if rc != MOM_OK:
        raise MomError(rc, lib.mom_last_global_error().decode())
    return sigma, dsigma.reshape(2, len(g)).T.copy()


def voigt_last_kernel_ms() -> float:
    return float(load().mom_voigt_last_kernel_ms())


def _mie_nai2(dual: bool, r, w, lam, n_r, n_i, w_mu, pi_tab, tau_tab, P, P2, R2, T2, flags, device):
    lib = load()
    name = "mie_nai2_dual" if dual else "mie_nai2"
    r, w, w_mu = f64(r), f64(np.atleast_2d(w)), f64(w_mu)
    tabs = [f64(np.asarray(t, dtype=np.float64).T) for t in (pi_tab, tau_tab, P, P2, R2, T2)]
    nW, nR, n_mu = w.shape[0], len(r), len(w_mu)
    if w.shape[1] != nR or any(t.shape[1] != n_mu for t in tabs) or tabs[0].shape != tabs[1].shape or \
            any(t.shape != tabs[2].shape for t in tabs[3:]):
        raise ValueError(f"{name}: array shapes do not agree")
    n_max, l_max = tabs[0].shape[0], tabs[2].shape[0]
    nO = nW + MOM_MIE_INDEX_ROWS if dual else nW
    bulk, Cx, greek, ms = np.empty((nO, 4, n_mu)), np.empty((nO, 2)), np.empty((nO, 6, l_max)), np.zeros(3)
    fn = lib.mom_mie_nai2_dual if dual else lib.mom_mie_nai2
    rc = fn(device, nR, dp(r), nW, dp(w), float(lam), float(n_r), float(n_i), n_mu, dp(w_mu), n_max, dp(tabs[0]), dp(tabs[1]), l_max,
            *[dp(t) for t in tabs[2:]], int(flags), dp(bulk), dp(Cx), dp(greek), dp(ms))
    if rc != MOM_OK:
        raise MomError(rc, lib.mom_last_global_error().decode())
    return bulk, Cx, greek, ms


def mie_nai2(r, w, lam, n_r, n_i, w_mu, pi_tab, tau_tab, P, P2, R2, T2, flags: int = 0, device: int = 0):
    """mom_mie_nai2: r [nR] ascending, w [nW, nR] weight rows, pi_tab / tau_tab [n_mu, n_max] and P, P2, R2, T2 [n_mu, l_max] as
    numpy builds them (the ABI's mu-fastest layout is their transpose).  Returns (bulk_f [nW, 4, n_mu], C [nW, 2],
    greek [nW, 6, l_max], gpu_ms [3]), all unnormalised."""
    return _mie_nai2(False, r, w, lam, n_r, n_i, w_mu, pi_tab, tau_tab, P, P2, R2, T2, flags, device)


def mie_nai2_dual(r, w, lam, n_r, n_i, w_mu, pi_tab, tau_tab, P, P2, R2, T2, flags: int = 0, device: int = 0):
    """mom_mie_nai2_dual: the arguments of mie_nai2 (nW <= 3); every output has nW + 2 rows, the last two the partials of row 0's
    sums with respect to n_r and n_i."""
    return _mie_nai2(True, r, w, lam, n_r, n_i, w_mu, pi_tab, tau_tab, P, P2, R2, T2, flags, device)


def mie_coefficients(x, n_r, n_i, n_max: int, device: int = 0):
    """mom_mie_coefficients: (a, b) complex [n_max, nX] for the size parameters x (row n - 1 = order n)."""
    lib = load()
    x = f64(np.atleast_1d(x))
    out = [np.empty((int(n_max), len(x))) for _ in range(4)]
    rc = lib.mom_mie_coefficients(device, len(x), dp(x), float(n_r), float(n_i), int(n_max), *[dp(o) for o in out])
    if rc != MOM_OK:
        raise MomError(rc, lib.mom_last_global_error().decode())
    return out[0] + 1j * out[1], out[2] + 1j * out[3]


def mie_coefficients_dual(x, n_r, n_i, n_max: int, device: int = 0):
    """mom_mie_coefficients_dual: (a, b, da/dm, db/dm) complex [n_max, nX]; d/dn_r = d/dm, d/dn_i = i d/dm."""
    lib = load()
    x = f64(np.atleast_1d(x))
    out = [np.empty((int(n_max), len(x))) for _ in range(8)]
    rc = lib.mom_mie_coefficients_dual(device, len(x), dp(x), float(n_r), float(n_i), int(n_max), *[dp(o) for o in out])
    if rc != MOM_OK:
        raise MomError(rc, lib.mom_last_global_error().decode())
    return out[0] + 1j * out[1], out[2] + 1j * out[3], out[4] + 1j * out[5], out[6] + 1j * out[7]


def mie_tables(mu, n_max: int, l_max: int, device: int = 0):
    """mom_mie_tables: (pi, tau [n_mu, n_max], P, P2, R2, T2 [n_mu, l_max]) of the nodes mu, built on the device, in the orientation
    numpy builds them in (scattering.compute_mie_π_τ, compute_legendre_poly): the transposes of the ABI's mu-fastest layout, so they
    go into mie_nai2 as they are."""
    lib = load()
    mu = f64(np.atleast_1d(mu))
    n_mu, n_max, l_max = len(mu), int(n_max), int(l_max)
    out = [np.empty((max(n_max, 0), n_mu)) for _ in range(2)] + [np.empty((max(l_max, 0), n_mu)) for _ in range(4)]
    rc = lib.mom_mie_tables(device, n_mu, dp(mu), n_max, l_max, *[dp(o) for o in out])
    if rc != MOM_OK:
        raise MomError(rc, lib.mom_last_global_error().decode())
    return tuple(o.T for o in out)


def _mie_nai2_spectral(dual: bool, r, w, lam, n_r, n_i, mu, w_mu, n_max, l_max, flags, max_batch, device):
    lib = load()
    name = "mie_nai2_spectral_dual" if dual else "mie_nai2_spectral"
    r, w, mu, w_mu = f64(r), f64(np.atleast_2d(w)), f64(mu), f64(w_mu)
    lam, n_r, n_i = (f64(np.atleast_1d(a)) for a in (lam, n_r, n_i))
    nW, nR, n_mu, nL, l_max = w.shape[0], len(r), len(w_mu), len(lam), int(l_max)
    if w.shape[1] != nR or len(mu) != n_mu or len(n_r) != nL or len(n_i) != nL:
        raise ValueError(f"{name}: array shapes do not agree")
    nO = nW + MOM_MIE_INDEX_ROWS if dual else nW
    bulk, Cx = np.empty((nL, nO, 4, n_mu)), np.empty((nL, nO, 2))
    greek, ms = np.empty((nL, nO, 6, max(l_max, 0))), np.zeros(4)
    fn = lib.mom_mie_nai2_spectral_dual if dual else lib.mom_mie_nai2_spectral
    rc = fn(device, nR, dp(r), nW, dp(w), nL, dp(lam), dp(n_r), dp(n_i), n_mu, dp(mu), dp(w_mu), int(n_max), l_max, int(flags),
            int(max_batch), dp(bulk), dp(Cx), dp(greek), dp(ms))
    if rc != MOM_OK:
        raise MomError(rc, lib.mom_last_global_error().decode())
    return bulk, Cx, greek, ms


def mie_nai2_spectral(r, w, lam, n_r, n_i, mu, w_mu, n_max: int, l_max: int, flags: int = 0, max_batch: int = 0, device: int = 0):
    """mom_mie_nai2_spectral: mie_nai2 for the wavelengths lam [nL] with the refractive indices n_r, n_i [nL] on ONE angle grid mu,
    w_mu, whose tables the device builds (n_max: their row count).  Returns (bulk_f [nL, nW, 4, n_mu], C [nL, nW, 2],
    greek [nL, nW, 6, l_max], gpu_ms [4]: tables, coefficients, GEMM with reduction, projection)."""
    return _mie_nai2_spectral(False, r, w, lam, n_r, n_i, mu, w_mu, n_max, l_max, flags, max_batch, device)


def mie_nai2_spectral_dual(r, w, lam, n_r, n_i, mu, w_mu, n_max: int, l_max: int, flags: int = 0, max_batch: int = 0, device: int = 0):
    """mom_mie_nai2_spectral_dual: as mie_nai2_spectral (nW <= 3) with nW + 2 rows per wavelength, the last two d/dn_r and d/dn_i"""
    return _mie_nai2_spectral(True, r, w, lam, n_r, n_i, mu, w_mu, n_max, l_max, flags, max_batch, device)


def mie_pcw(r, w, lam, n_r, n_i, N_max: int, flags: int = 0, device: int = 0):
    """mom_mie_pcw: r [nR] ascending, w [nR] = w_x.  Returns (greek [6, 2 N_max - 1] not divided by C_sca, C [2] = (C_sca, C_ext),
    gpu_ms [3])."""
    lib = load()
    r, w = f64(r), f64(w)
    if r.ndim != 1 or w.shape != r.shape:
        raise ValueError("mie_pcw: r and w must be vectors of one length")
    N_max = int(N_max)
    greek, Cx, ms = np.empty((6, max(2 * N_max - 1, 1))), np.empty(2), np.zeros(3)
    rc = lib.mom_mie_pcw(device, len(r), dp(r), dp(w), float(lam), float(n_r), float(n_i), N_max, int(flags), dp(greek), dp(Cx), dp(ms))
    if rc != MOM_OK:
        raise MomError(rc, lib.mom_last_global_error().decode())
    return greek, Cx, ms


def wigner_tables(m_max: int, n_max: int, l_max: int, device: int = 0):
    """mom_wigner_tables: (wigner_A, wigner_B), each indexed [m - 1, n - 1, l - 1] like the reference's arrays (views of the ABI's
    m-fastest layout: column-major, as Julia holds them)."""
    lib = load()
    m_max, n_max, l_max = int(m_max), int(n_max), int(l_max)
    ok = min(m_max, n_max, l_max) >= 1 and m_max * n_max * l_max * 8 <= MOM_WIGNER_MAX_TABLE_BYTES
    out = [np.empty((l_max, n_max, m_max) if ok else (1,)) for _ in range(2)]   # a refused size is refused by the library, unallocated
    rc = lib.mom_wigner_tables(device, m_max, n_max, l_max, dp(out[0]), dp(out[1]))
    if rc != MOM_OK:
        raise MomError(rc, lib.mom_last_global_error().decode())
    return out[0].transpose(2, 1, 0), out[1].transpose(2, 1, 0)


def pcw_pair_averages(r, w, lam, n_r, n_i, N_max: int, device: int = 0):
    """mom_pcw_pair_averages: (anam, anbm, bnam, bnbm) complex [N_max, N_max], entry [m - 1, n - 1] for m >= n."""
    lib = load()
    r, w = f64(r), f64(w)
    if r.ndim != 1 or w.shape != r.shape:
        raise ValueError("pcw_pair_averages: r and w must be vectors of one length")
    N_max = int(N_max)
    out = [np.empty((max(N_max, 1), max(N_max, 1))) for _ in range(8)]
    rc = lib.mom_pcw_pair_averages(device, len(r), dp(r), dp(w), float(lam), float(n_r), float(n_i), N_max, *[dp(o) for o in out])
    if rc != MOM_OK:
        raise MomError(rc, lib.mom_last_global_error().decode())
    return tuple(out[2 * q] + 1j * out[2 * q + 1] for q in range(4))


def _pcw_dual_args(fn: str, r, w, index_rows: bool):
    r, w = f64(r), f64(w)
    if w.ndim == 1:
        w = w[None, :]
    if r.ndim != 1 or w.ndim != 2 or w.shape[1] != r.shape[0]:
        raise ValueError(f"{fn}: r [nR] must be a vector and w [nW, nR] its weight rows")
    nO = w.shape[0] + (2 if index_rows else 0)
    return r, np.ascontiguousarray(w), nO, MOM_PCW_INDEX_ROWS if index_rows else 0


def mie_pcw_dual(r, w, lam, n_r, n_i, N_max: int, index_rows: bool = False, device: int = 0, flags=None):
    """mom_mie_pcw_dual: r [nR] ascending, w [nW, nR], row 0 = w_x, further rows its partials.  Returns (greek [nO, 6, 2 N_max - 1]
    not divided by C_sca, C [nO, 2], gpu_ms [3]), nO = nW + 2 with index_rows: then the last two rows are d/dn_r and d/dn_i of row
    0.  flags (test access) replaces the flag word index_rows stands for."""
    lib = load()
    r, w, nO, fl = _pcw_dual_args("mie_pcw_dual", r, w, index_rows)
    N_max = int(N_max)
    greek, Cx, ms = np.empty((nO, 6, max(2 * N_max - 1, 1))), np.empty((nO, 2)), np.zeros(3)
    rc = lib.mom_mie_pcw_dual(device, len(r), dp(r), w.shape[0], dp(w), float(lam), float(n_r), float(n_i), N_max,
                              fl if flags is None else int(flags), dp(greek), dp(Cx), dp(ms))
    if rc != MOM_OK:
        raise MomError(rc, lib.mom_last_global_error().decode())
    return greek, Cx, ms


def pcw_pair_averages_dual(r, w, lam, n_r, n_i, N_max: int, index_rows: bool = False, device: int = 0):
    """mom_pcw_pair_averages_dual: complex [nO, 4, N_max, N_max]: per row (anam, anbm, bnam, bnbm), entry [m - 1, n - 1] for m >= n."""
    lib = load()
    r, w, nO, fl = _pcw_dual_args("pcw_pair_averages_dual", r, w, index_rows)
    N_max = int(N_max)
    out = np.empty((nO, 8, max(N_max, 1), max(N_max, 1)))
    rc = lib.mom_pcw_pair_averages_dual(device, len(r), dp(r), w.shape[0], dp(w), float(lam), float(n_r), float(n_i), N_max, fl, dp(out))
    if rc != MOM_OK:
        raise MomError(rc, lib.mom_last_global_error().decode())
    return out[:, 0::2] + 1j * out[:, 1::2]


def pack_greeks(greeks, fn: str):
    """Greek sets (each six vectors α, β, γ, δ, ϵ, ζ of the set's own length) as the ABI's (nG, l_pad, l_max [nG], greek [nG, 6, l_pad])."""
    rows = [[f64(r) for r in g] for g in greeks]
    if any(len(g) != 6 or any(r.ndim != 1 or r.shape != g[0].shape for r in g) for g in rows):
        raise ValueError(f"{fn}: mu must be a vector and every Greek set six vectors of one length")
    nG = len(rows)
    l_max = i32([len(g[0]) for g in rows])
    l_pad = max(int(l_max.max()) if nG else 1, 1)
    greek = np.zeros((max(nG, 1), 6, l_pad))
    for k, g in enumerate(rows):
        for q in range(6):
            greek[k, q, :len(g[q])] = g[q]
    return nG, l_pad, l_max, greek


def z_moments(nStokes: int, mu, greeks, M: int, m_first: int = 0, set_inner: int = 0, device: int = 0):
    """mom_z_moments: Z⁺⁺, Z⁻⁺ of the Greek sets `greeks` (each a sequence of the six rows α, β, γ, δ, ϵ, ζ, of the set's own length)
    at the nodes mu for the moments m_first .. m_first + M - 1.  Returns (Zpp, Zmp, gpu_ms): the ABI buffers as C arrays
    [M, nG, N(j), N(i)] for set_inner = 0, and [P, M, K, N(j), N(i)] for set_inner = K (sets ordered g = k + K p, the dZpp / dZmp
    layout of mom_scene_set_partials)."""
    lib = load()
    mu = f64(mu)
    rows = [[f64(r) for r in g] for g in greeks]
    nG, M, m_first, set_inner = len(rows), int(M), int(m_first), int(set_inner)
    if mu.ndim != 1:
        raise ValueError("z_moments: mu must be a vector and every Greek set six vectors of one length")
    _, l_pad, l_max, greek = pack_greeks(rows, "z_moments")
    N = int(nStokes) * len(mu)
    ok = nG >= 1 and M >= 1 and N >= 1 and set_inner >= 0 and (set_inner == 0 or nG % set_inner == 0)
    shape = ((M, nG, N, N) if set_inner == 0 else (nG // set_inner, M, set_inner, N, N)) if ok else (1,)   # a refused size is refused by the library
    Zpp, Zmp, ms = np.empty(shape), np.empty(shape), np.zeros(1)
    rc = lib.mom_z_moments(device, int(nStokes), len(mu), dp(mu), nG, l_pad, ip(l_max), dp(greek), m_first, M, set_inner, dp(Zpp), dp(Zmp),
                           dp(ms))
    if rc != MOM_OK:
        raise MomError(rc, lib.mom_last_global_error().decode())
    return Zpp, Zmp, float(ms[0])


TRUNCATE_MAX = 128   # the largest truncation order of mom_truncate_phase


def truncate_phase(mu, w_mu, greek, l_tr: int, device: int = 0):
    """mom_truncate_phase: greek [nG, 1 + nP, 6, l_full] (the ABI's array as a C array: sets, then the set and its nP derivative sets,
    then the rows α, β, γ, δ, ϵ, ζ) truncated to l_tr terms at the nodes mu with weights w_mu.  Returns (greek_t [nG, 1 + nP, 6, l_tr],
    c0 [nG, 1 + nP], status [nG], gpu_ms).  A set whose status word is not zero has NaN rows and is not an error of this wrapper:
    MOM_ESINGULAR comes back as the status array, every other code raises MomError."""
    lib = load()
    mu, w_mu, greek = f64(mu), f64(w_mu), f64(greek)
    if mu.ndim != 1 or w_mu.shape != mu.shape or greek.ndim != 4 or greek.shape[2] != 6:
        raise ValueError("truncate_phase: mu and w_mu must be vectors of one length and greek [nG, 1 + nP, 6, l_full]")
    nG, R, _, l_full = greek.shape
    l_tr = int(l_tr)
    ok = nG >= 1 and R >= 1 and 1 <= l_tr <= l_full
    greek_t = np.empty((nG, R, 6, l_tr) if ok else (1,))   # a refused size is refused by the library
    c0, status, ms = np.empty((max(nG, 1), max(R, 1))), np.zeros(max(nG, 1), dtype=np.int32), np.zeros(1)
    rc = lib.mom_truncate_phase(device, len(mu), dp(mu), dp(w_mu), nG, R - 1, l_full, l_tr, dp(greek), dp(greek_t), dp(c0), ip(status),
                                dp(ms))
    if rc not in (MOM_OK, MOM_ESINGULAR):
        raise MomError(rc, lib.mom_last_global_error().decode())
    return greek_t, c0, status, float(ms[0])
