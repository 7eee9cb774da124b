// gconvx_f16.hip - fp16 instantiations of the any-width grouped 3x3 kernel (gconvx.hpp)
#include "gconvx.hpp"
GCONVX_INSTANCES(GCONVX_DEFINE, PCV_F16)
