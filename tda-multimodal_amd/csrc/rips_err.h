// rips_err.h -- error flags a kernel ORs into LayerStats::err, read by the host after the
// call's one synchronisation.  Plain C++ (no HIP): rips_retry.h decides the next attempt on them.
#pragma once
#include <stdint.h>

namespace tda {

enum : int32_t {
    ERR_RESID_CAP = 1,
    ERR_PAIR_CAP = 2,
    ERR_WORK_CAP = 4,
    ERR_VPOOL_CAP = 8,
    ERR_OUT_CAP = 16,
    ERR_LDS_SPILL = 32,
    ERR_STEP_LIMIT = 64,  // a column exceeded the pivot budget
    // k_reduce_par aborted: the host re-runs the call with k_reduce_big (ERR_PAR:
    // the H1 launch aborted, both dimensions go serial; ERR_PAR2: the H2 launch
    // aborted, H1 stays parallel and H2 goes serial).  ERR_CAP_MISS (per layer): a
    // capped column ran empty below its cap; the layer's remaining columns are
    // dropped and the host re-runs that layer alone without caps.
    ERR_PAR = 128,
    ERR_PAR2 = 256,
    ERR_CAP_MISS = 512,
};

}  // namespace tda
