// mixconv_bf16.hip - bf16 instantiations of the depthwise MixConv kernel (mixconv.hpp)
#include "mixconv.hpp"
MIX_INSTANCES(MIX_DEFINE, PCV_BF16)
