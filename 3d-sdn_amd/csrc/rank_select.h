// The rank search over a 256-bin histogram.  The exact radix select of the disparity percentile calls it from k_ids_select and
// k_ids_pick (scene_ids.hip), which serve both sdn_scene_id_stats (a row per id of one frame) and sdn_train_id_stats (a row per
// item of a batch): those kernels live in that one source, so each is defined once in the library, and this header holds no
// kernel.  The top-k selects of proposal_layer.hip and rpn_targets.hip call it too.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_common.h"

namespace sdn {

// The bin of a 256-bin histogram that holds the element of rank `rank` (zero-based, ascending) and the rank inside that bin,
// by one wave: four bins per lane, an exclusive scan over the lanes.  (0, 0) when the histogram holds fewer elements.
__device__ __forceinline__ void ids_find(const int32_t* hist, long rank, int lane, int* bin, int* residual)
{
    int c[4];
    int sum = 0;
    for (int k = 0; k < 4; k++) {
        c[k] = hist[4 * lane + k];
        sum += c[k];
    }
    int total;   // not needed: a rank past every bin finds nothing
    const int below = wave_exclusive_sum(sum, lane, total);
    const int incl = below + sum;
    long before = below;
    int b = 0, r = 0;
    bool found = false;
    if (rank >= before && rank < incl) {
        for (int k = 0; k < 4 && !found; k++) {
            if (rank < before + c[k]) {
                found = true;
                b = 4 * lane + k;
                r = (int)(rank - before);
            }
            before += c[k];
        }
    }
    const unsigned long long m = __ballot(found);
    const int src = m ? __ffsll((long long)m) - 1 : 0;
    *bin = __shfl(b, src, 64);
    *residual = __shfl(r, src, 64);
}

}  // namespace sdn
