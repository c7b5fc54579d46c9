"""parallel_finite_difference_computation_amd -- MI355X (gfx950) 2-D acoustic finite-difference /
RTM hot path behind the reference's own interfaces.  The compute lives in libfdwave.so
(csrc/: hand-written HIP kernels + C ABI, include/fdwave.h); this package is the thin host side.
Importing the package does not touch the GPU; using it without libfdwave.so raises ImportError.
"""
from ._lib import BORN_DTT, BORN_FIELD, IMAGE_DTT, IMAGE_XCORR, FdwError, LIB_PATH, MODE_FWD, MODE_PLAIN, MODE_RECV, lib  # noqa: F401
from .api import (FDWave, calc_coefs, extendvel_linear, fd_back, fd_forward, fd_init, image_compare, gather_misfit, gather_scale_v2, image_unscale_v2, image_compensate, image_excitation, image_laplacian, mod_extendvel,  # noqa: F401
                  mod_ricker_wavelet, mod_taper_tables, ricker_wavelet, snap_dims, srand, taper_tables, planewave_lags, encode_line_source, encode_gathers, encode_gathers_multi, plan_pass_bands, plan_pass_cut, plan_ext_image)

from .slabs import Comm, Slabs, run_ranks  # noqa: F401,E402

__all__ = ["Comm", "Slabs", "run_ranks", "FDWave", "FdwError", "calc_coefs", "ricker_wavelet", "taper_tables", "extendvel_linear", "srand",
           "fd_init", "fd_forward", "fd_back", "mod_extendvel", "mod_ricker_wavelet", "mod_taper_tables", "image_laplacian", "image_compare", "image_compensate", "image_excitation", "gather_misfit", "snap_dims", "planewave_lags", "encode_line_source", "encode_gathers", "encode_gathers_multi", "plan_pass_bands", "plan_pass_cut", "plan_ext_image", "lib", "LIB_PATH", "MODE_FWD", "MODE_PLAIN", "MODE_RECV", "BORN_FIELD", "BORN_DTT", "IMAGE_XCORR", "IMAGE_DTT", "gather_scale_v2", "image_unscale_v2"]
