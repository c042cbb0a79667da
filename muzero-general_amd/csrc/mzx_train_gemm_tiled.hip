// mzx_train_gemm_tiled.hip -- the six instantiations of the residual trainer's LDS-tiled GEMM (mzx_train_gemm_tiled.h:
// forward, input gradient, weight gradient, each in both precisions) behind rtn_launch_tiled, in a translation unit of
// their own: build.py compiles it without the packed binary32 instructions.
#include <hip/hip_runtime.h>

#define MZX_TRAIN_GEMM_TILED_DEFINE
#include "mzx_train_gemm_tiled.h"
