// fp8 (OCP e4m3) operand tiles of the implicit-GEMM kernel (igemm_kernel.h).
#include "igemm_plan.h"

// fp8 operands: the F_F8 subset of the dense tiles (no split-K: the slab reduce does not carry the operand scales)
int pbe_dispatch_f8(IGemmP p, int batch, hipStream_t s, int want_cfg) {
    p.ws = nullptr;                                   // no workspace: splits_for() returns 1 for every tile
    const Plan pl = plan_igemm(p, batch, 0, want_cfg, 0);
    p.splits = 1;
    return launch_tile<F_F8, 0, true>(pl.cfg, p, batch, s);
}

// the same tiles with the MX-fp8 copy-out (pbe_gemm_mx8out_f16: q | k, or V^T from the swapped projection)
int pbe_launch_f8_mx8(int cfg, IGemmP p, int batch, hipStream_t s) { return launch_tile<F_F8, 0, true, EX_MX>(cfg, p, batch, s); }
