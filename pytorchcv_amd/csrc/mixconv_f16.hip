// mixconv_f16.hip - f16 instantiations of the depthwise MixConv kernel (mixconv.hpp)
#include "mixconv.hpp"
MIX_INSTANCES(MIX_DEFINE, PCV_F16)
