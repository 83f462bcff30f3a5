// attention2.hip compiled a second time on IEEE-half elements: dk_f16::dk_attn2_fwd_kernel<64, 4, false, QFUSE>, under the flags of the
// bf16 D = 64 forms (Makefile).
#define DK_ELEM_F16 1
#include "dk_kernels.h"
namespace dk_f16 {
#include "attention2.hip"
}
