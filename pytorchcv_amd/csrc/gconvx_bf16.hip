// gconvx_bf16.hip - bf16 instantiations of the any-width grouped 3x3 kernel (gconvx.hpp)
#include "gconvx.hpp"
GCONVX_INSTANCES(GCONVX_DEFINE, PCV_BF16)
