// Extended-epilogue dense tiles of the implicit-GEMM kernel (igemm_kernel.h): every feature (combinations outside the three the transformer block uses).
#include "igemm_plan.h"

int pbe_launch_ex_all(int cfg, IGemmP p, int batch, hipStream_t s) { return launch_tile<F_EX, 0, false, EX_LN | EX_ST | EX_VT>(cfg, p, batch, s); }
