// bnu_16bit.hip - bf16 and fp16 instantiations of the fused stage-1 bottleneck unit (plain and identity-convolution form)
#include "bnu.hpp"
template __global__ void bnu_kernel<PCV_BF16, false>(const BnuParams);
template __global__ void bnu_kernel<PCV_BF16, true>(const BnuParams);
template __global__ void bnu_kernel<PCV_F16, false>(const BnuParams);
template __global__ void bnu_kernel<PCV_F16, true>(const BnuParams);
