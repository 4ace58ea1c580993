"""ginsim -- MI355X-native Monte-Carlo strapdown-INS engine (host side of libginsim.so).

Importing this package loads the HIP library through ctypes; it raises if the library has not been
built.  There is no CPU implementation behind it.
"""
from ._lib import lib, LIB_PATH, EXPORTS, OALLAN_EXPORTS, PSD_EXPORTS, LPSD_EXPORTS, CSD_EXPORTS, LOOSE_ALL_EXPORTS, LOOSE_ALL_CONS_EXPORTS, GinsimError, GinsimOutOfMemory, PlacedUnavailable, ALGO_FREE, ALGO_ODO          # noqa: F401
from .engine import (Context, DeviceBuffer, MonteCarloJob, AuxSensorJob, StatsResult, CurveResult, CovResult, track_frame, error_ellipse, QuantileResult, quantile_rows, ConsistencyResult, device_count, pathgen, pinned_empty, vibration, psd_amplitudes,  # noqa: F401
                     sensor_model, ini_table, free_integration_host, rng_normals, normal_transform, default_context, allan_var, allan_var_host, allan_plan, ALLAN_MODES,
                     oallan_var, oallan_var_host, oallan_plan, OALLAN_FORMS,
                     welch_psd, welch_psd_host, welch_plan, PSD_WINDOWS,
                     lpsd, lpsd_host, lpsd_plan, decimate2, model_psd,
                     welch_csd, welch_csd_host, csd_plan, CsdResult)
from .inclinometer import InclinometerJob  # noqa: F401,E402
from .magcal import MagCalJob  # noqa: F401,E402
from .ins_loose import InsLooseJob, filter_model, aiding_model, mag_model, scale_model, still_model, standstill_flags  # noqa: F401,E402
