"""spx_amd -- MI355X-native shifted proximal operators (the prox! hot path of
ShiftedProximalOperators.jl) behind the reference's own API.  The directory is named
`shiftedproximaloperators.jl_amd`; import it as `spx_amd` through the loader at the repository root."""
from . import _lib
from ._lib import SpxError
from .functions import (GroupNormL2, IndBallL0, NormL0, NormL1, NormL2, NormLinf, ProximableFunction,
                        RootNormLhalf)
from .sharding import shard_range
from .shifted import (ShiftedGroupNormL2, ShiftedGroupNormL2Binf, ShiftedIndBallL0, ShiftedIndBallL0BInf,
                      ShiftedNormL0, ShiftedNormL0Box, ShiftedNormL1, ShiftedNormL1B2, ShiftedNormL1Box,
                      ShiftedProximableFunction, ShiftedRootNormLhalf, ShiftedRootNormLhalfBox, b2_prox_step, b2_prox_step_bang,
                      context, device_values,
                      group_prox_step, group_prox_step_bang, iprox, iprox_bang, iprox_step, iprox_step_bang,
                      iprox_step_batch, iprox_step_batch_bang, lhalf_threshold_batch, prox,
                      prox_step_lhalf_batch, prox_step_lhalf_batch_bang,
                      prox_bang, prox_step, prox_step_b2_batch, prox_step_b2_batch_bang, prox_step_bang, prox_step_batch, prox_step_batch_bang,
                      prox_step_group_batch, prox_step_group_batch_bang, prox_step_group_binf_batch,
                      prox_step_group_binf_batch_bang, prox_step_topr_batch, prox_step_topr_batch_bang, prox_value, prox_value_bang, set_bounds_bang, set_radius_bang, shift_bang, shifted, synchronize, value)

__all__ = [n for n in dir() if not n.startswith("_")]
