// mzx_train_gemm_ksplit.hip -- the six instantiations of the residual trainer's in-workgroup split-K GEMM
// (mzx_train_gemm_ksplit.h: forward, input gradient, weight gradient, each in both precisions) behind rtn_launch_ksplit, in a
// translation unit of their own: build.py compiles it without the packed binary32 instructions.
#include <hip/hip_runtime.h>

#define MZX_TRAIN_GEMM_KSPLIT_DEFINE
#include "mzx_train_gemm_ksplit.h"
