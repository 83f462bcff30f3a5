// vae_ops.hip compiled a second time on IEEE-half elements: GroupNorm partials / statistics / apply / table (gamma and beta in fp16, sums in
// fp32), row softmax, transpose, channel padding, the image tail and the encoder's moment kernels.
#define DK_ELEM_F16 1
#include "dk_kernels.h"
namespace dk_f16 {
#include "vae_ops.hip"
}
