// gemm.hip compiled a second time on IEEE-half elements: dk_f16::dk_gemm_bf16_kernel<0> and its launcher (dk_common.h, element-type layer).
#define DK_ELEM_F16 1
#include "dk_kernels.h"
namespace dk_f16 {
#include "gemm.hip"
}
