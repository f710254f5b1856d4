// Extended-epilogue dense tiles of the implicit-GEMM kernel (igemm_kernel.h): row statistics out (proj_in, attention out-projection).
#include "igemm_plan.h"

int pbe_launch_ex_st(int cfg, IGemmP p, int batch, hipStream_t s) { return launch_tile<F_EX, 0, false, EX_ST>(cfg, p, batch, s); }
