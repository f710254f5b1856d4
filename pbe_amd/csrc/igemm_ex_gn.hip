// Extended-epilogue dense tiles of the implicit-GEMM kernel (igemm_kernel.h): GroupNorm folded into the A fragments, row statistics out
// (the SpatialTransformer's proj_in; pbe_gemm_gnfold_f16).
#include "igemm_plan.h"

int pbe_launch_ex_gn(int cfg, IGemmP p, int batch, hipStream_t s) { return launch_tile<F_EX, 0, false, EX_ST | EX_GN>(cfg, p, batch, s); }
