// Extended-epilogue dense tiles of the implicit-GEMM kernel (igemm_kernel.h): LayerNorm folded in + q pre-scale + V^T tiles (the fused q | k | v projection).
#include "igemm_plan.h"

int pbe_launch_ex_qkv(int cfg, IGemmP p, int batch, hipStream_t s) { return launch_tile<F_EX, 0, false, EX_LN | EX_VT>(cfg, p, batch, s); }
// the same tiles with the MX-fp8 copy-out (pbe_gemm_mx8out_f16): q | k | V^T leave as pbe_attention_mx8's operands
int pbe_launch_ex_qkv_mx8(int cfg, IGemmP p, int batch, hipStream_t s) { return launch_tile<F_EX, 0, false, EX_LN | EX_VT | EX_MX>(cfg, p, batch, s); }
