// Halo-resident 3x3 conv (MODE 2) tiles of the implicit-GEMM kernel (igemm_kernel.h).
#include "igemm_plan.h"

int pbe_launch_halo(int cfg, IGemmP p, int batch, hipStream_t s) { return launch_tile<F_HALO, 2>(cfg, p, batch, s); }
