// Dense (MODE 0) tiles of the implicit-GEMM kernel (igemm_kernel.h).
#include "igemm_plan.h"

int pbe_dispatch_dense(IGemmP p, int batch, hipStream_t s, size_t ws_bytes, int want_cfg) {
    const Plan pl = plan_igemm(p, batch, ws_bytes, want_cfg, 0);
    p.splits = pl.splits;
#ifdef PBE_STAMPS
    p.stamps = g_pbe_stamps;
#endif
    return launch_tile<F_DENSE, 0>(pl.cfg, p, batch, s);
}
