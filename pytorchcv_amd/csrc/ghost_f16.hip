// ghost_f16.hip - f16 instantiations of the ghost-module kernel (ghost.hpp)
#include "ghost.hpp"
GHOST_INSTANCES(GHOST_DEFINE, PCV_F16)
