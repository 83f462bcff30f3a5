// elementwise.hip compiled a second time on IEEE-half elements: the kernels the MMDiT engine and the step loop launch.
#define DK_ELEM_F16 1
#include "dk_kernels.h"
namespace dk_f16 {
#include "elementwise.hip"
}
