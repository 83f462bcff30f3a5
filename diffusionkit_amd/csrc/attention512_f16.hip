// attention512.hip compiled a second time on IEEE-half elements, under the flags of its bf16 twin (Makefile): scores, running maximum and
// sum stay fp32, P is rounded to fp16 for the P.V MFMA (P <= e^4 under the deferred rescale: far inside fp16's range).
#define DK_ELEM_F16 1
#include "dk_kernels.h"
namespace dk_f16 {
#include "attention512.hip"
}
