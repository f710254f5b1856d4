// Extended-epilogue dense tiles of the implicit-GEMM kernel (igemm_kernel.h): LayerNorm folded in (the GEGLU projection).
#include "igemm_plan.h"

int pbe_launch_ex_ln(int cfg, IGemmP p, int batch, hipStream_t s) { return launch_tile<F_EX, 0, false, EX_LN>(cfg, p, batch, s); }
