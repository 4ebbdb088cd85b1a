"""MI355X-native Matrix-Operator RT core (drop-in for vSmartMOM.jl's CoreRT hot path).

The directory name contains a dot, so import it through the root-level shim:
    import rtamd            # -> this package, registered as module "rtamd"
"""
from . import _lib  # noqa: F401
from ._lib import Handle, MomError, voigt_xsec, voigt_xsec_dual, load  # noqa: F401
from . import corert, scenes, absorption, sharding, scattering  # noqa: F401,E402
from .absorption import (Range, InterpolationModel, make_interpolation_model, interpolation_model_from_table,  # noqa: F401,E402
                         save_interpolation_model, load_interpolation_model)
from .corert import (MI355X, rt_run, rt_run_dual, ScenePartial, OpticsPartial, rt_run_dual_device_optics, rt_run_test_ms, rt_run_operators, model_from_parameters, prepare_scene, compute_Z_moments, compute_Z_moments_batch, z_bases,  # noqa: F401,E402
                     vSmartMOM_Parameters, vSmartMOM_Model, Bands, with_bands, Stokes_I, Stokes_IQU, Stokes_IQUV)
from .scattering import (LogNormal, Aerosol, NAI2, PCW, δBGE, make_mie_model, compute_wigner_values, compute_aerosol_optical_properties,  # noqa: F401,E402
                         compute_spectral_aerosol_optical_properties, spectral_mie_inputs,
                         compute_ref_aerosol_extinction, truncate_phase, truncate_phase_batch, ALL_AEROSOL_PARAMETERS, aerosol_derivs,
                         aerosol_optics_partial, aerosol_optics_partials, band_aerosol_optics, aerosol_optics_jacobian)
