// ghost_bf16.hip - bf16 instantiations of the ghost-module kernel (ghost.hpp)
#include "ghost.hpp"
GHOST_INSTANCES(GHOST_DEFINE, PCV_BF16)
