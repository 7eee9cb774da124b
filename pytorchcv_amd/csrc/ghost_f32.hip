// ghost_f32.hip - f32 instantiations of the ghost-module kernel (ghost.hpp)
#include "ghost.hpp"
GHOST_INSTANCES(GHOST_DEFINE, PCV_F32)
