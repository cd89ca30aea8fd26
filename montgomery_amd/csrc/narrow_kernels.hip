// The digit kernels of narrow scalars (msm_run_narrow) and k_scalar_bits: their one definition.
#include <hip/hip_runtime.h>
#define MSM_NARROW_TU 1
#include "narrow_kernels.h"
