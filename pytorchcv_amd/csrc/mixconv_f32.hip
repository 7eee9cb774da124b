// mixconv_f32.hip - f32 instantiations of the depthwise MixConv kernel (mixconv.hpp)
#include "mixconv.hpp"
MIX_INSTANCES(MIX_DEFINE, PCV_F32)
