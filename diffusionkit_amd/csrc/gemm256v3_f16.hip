// gemm256v3.hip compiled a second time on IEEE-half elements: dk_f16::dk_gemm256v3_kernel<MF, false> (every epilogue, the grouped launch, the
// row maps, the half column tile, the fused QKNorm tail and the K split, whose fp32 accumulator exchange does not see the element type).
#define DK_ELEM_F16 1
#include <cstring>
#include <type_traits>
#include "dk_kernels.h"
namespace dk_f16 {
#include "gemm256v3.hip"
}
