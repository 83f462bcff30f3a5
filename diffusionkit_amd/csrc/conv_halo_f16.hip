// conv_halo.hip compiled a second time on IEEE-half elements: dk_f16::dk_conv_halo_kernel<128, false> / <16, true> and their launcher (the
// GroupNorm-apply -> SiLU -> 3x3 conv with shortcut extension, nearest-x2 view, output statistics and image tail).  No asm frame behind it.
#define DK_ELEM_F16 1
#include "dk_kernels.h"
namespace dk_f16 {
#include "conv_halo.hip"
}
