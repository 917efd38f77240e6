// The bilinear sample of crop_and_resize (geometric/maskrcnn/roialign/roi_align/src/crop_and_resize.c:43-106), shared by the per-element
// kernels of raster_boxes.hip and the per-box sample table of pyramid_roi_align.hip, so that both give the bits of the reference's C.
// Device code only; the files that include it are built without FMA contraction.
#pragma once
#include <hip/hip_runtime.h>

namespace sdn {

// crop_and_resize.c:43-58: source coordinate of output index k along one axis (float / double mixing as written there)
__device__ __forceinline__ float axis_in(float a1, float a2, int extent, int crop, int k)
{
    if (crop > 1) {
        const float scale = (a2 - a1) * (float)(extent - 1) / (float)(crop - 1);
        return a1 * (float)(extent - 1) + (float)k * scale;
    }
    return (float)(0.5 * (double)(a1 + a2) * (double)(extent - 1));
}

// crop_and_resize.c:58, 80 turned round: a sample outside the map takes the extrapolation value and passes no gradient.  For every
// number this is !(in < 0 || in > extent - 1) as written there; a NaN coordinate, with which the C code goes on to index the map by
// an undefined int, counts as outside here.
__device__ __forceinline__ bool axis_inside(float in, int extent) { return in >= 0 && in <= (float)(extent - 1); }

}  // namespace sdn
