// 3x3 conv gather (MODE 1) tiles of the implicit-GEMM kernel (igemm_kernel.h).
#include "igemm_plan.h"

int pbe_dispatch_conv(IGemmP p, int batch, hipStream_t s, size_t ws_bytes, int want_cfg) {
    const Plan pl = plan_igemm(p, batch, ws_bytes, want_cfg, 1);
    p.splits = pl.splits;
#ifdef PBE_STAMPS
    p.stamps = g_pbe_stamps;
#endif
    if (kTiles[pl.cfg].forms & F_HALO) return pbe_launch_halo(pl.cfg, p, batch, s);      // halo-resident tiles: igemm_halo.hip
    return launch_tile<F_CONV, 1>(pl.cfg, p, batch, s);
}
