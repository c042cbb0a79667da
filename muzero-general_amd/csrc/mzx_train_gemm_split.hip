// mzx_train_gemm_split.hip -- the six instantiations of the residual trainer's split-BF16 tiled GEMM (mzx_train_gemm_split.h:
// forward, input gradient, weight gradient, each in both precisions) behind rtn_launch_split, in a translation unit of
// their own: build.py compiles it without the packed binary32 instructions.
#include <hip/hip_runtime.h>

#define MZX_TRAIN_GEMM_SPLIT_DEFINE
#include "mzx_train_gemm_split.h"
