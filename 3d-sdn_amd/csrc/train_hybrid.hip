// The training items of the real-image sets and of the hybrid batches of the geometric branch (geometric/derender3d/
// datasets.py:549-606 KittiObject, :737-769 KittiSemantics, :930-971 CityscapesSemantics, :1077-1112 CityscapesMaskRCNN beside
// :332-420 VKitti; data_loader.py:17-37 collate_fn).  A batch mixes frames of several sizes, two normalisations, masks from a
// colour code or from an instance-id map, and ignore maps from nearer codes, from a disparity percentile, or all zero.
//   sdn_train_id_stats      the area, box and disparity percentile of B (frame, id) items: one exact radix select with
//                           sdn_scene_id_stats, and defined beside it in scene_ids.hip.
//   sdn_train_crops_mixed   the kernel body of k_train_crops (train_items_common.h: ti_crops_body, instantiated here on a
//                           per-item source) with every per-call quantity moved into the item row: the frame's address and
//                           size, the sources of the mask and of the ignore map, mean and std.  A plane without a source is
//                           written as 0.0 by its workgroups, without staging.  The window, the colour-code test and the
//                           jitter (read from the MixItem itself) are train_items_common.h's; only the id-map mask and the
//                           disparity ignore map are written here.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sdn_common.h"
#include "train_hybrid_check.h"
#include "train_items_common.h"

namespace sdn {

static_assert(MX_SRC_PIXELS == TI_SRC_PIXELS && MX_PLANE_BYTES == TI_PLANE_BYTES && MX_MAX_CONTRAST_SIDE == TI_MAX_CONTRAST_SIDE &&
              MX_OBJ_INTS == TI_OBJ_INTS, "the validator's constants are the kernels'");

struct MixParams {
    const TrainWin* objs;
    const MixItem* items;
    const int32_t* bounds;
    const int32_t* kk8;
    const uint8_t* nearer;     // [total, 3]
    unsigned long long* lsum;  // [B] sum of L over the window (items with contrast)
    int B, Si, Sm;
    float *images, *masks, *ignores;
};

// the window's pixels of the ITEM's frame; beside train_items.hip's sources, a mask from an id map and an ignore map from disparity
struct MixSrc {
    const MixParams& A;
    const MixItem& it;
    const TrainWin& o;
    __device__ __forceinline__ void rgb(int wy, int wx, int& r, int& g, int& b) const
    {
        ti_raw_rgb(o, reinterpret_cast<const uint8_t*>(it.frame), it.H, it.W, wy, wx, r, g, b);
    }
    // the plane's source kind is not 0 (the caller wrote such a plane as zeros)
    __device__ __forceinline__ int map_byte(int kind, int wy, int wx) const
    {
        size_t p = 0;
        const int v = ti_map_outside(o, it.H, it.W, kind, wy, wx, &p);
        if (v >= 0) return v;
        if (kind == 1 && it.mask_kind != MX_MASK_CODE) return reinterpret_cast<const int32_t*>(it.mask_src)[p] == it.code ? 255 : 0;
        if (kind == 2 && it.ignore_kind == MX_IGNORE_DISPARITY) return reinterpret_cast<const int32_t*>(it.ignore_src)[p] > it.thr ? 255 : 0;
        return ti_code_byte(reinterpret_cast<const uint8_t*>(kind == 1 ? it.mask_src : it.ignore_src), p, kind, it.code,
                            A.nearer + 3 * (size_t)it.near_off, it.near_cnt);
    }
    __device__ __forceinline__ float mean(int ch) const { return it.mean[ch]; }
    __device__ __forceinline__ float stdev(int ch) const { return it.std[ch]; }
};

__global__ __launch_bounds__(TI_THREADS) void k_train_stats_mixed(const MixParams A)
{
    __shared__ int s_part[TI_WAVES];
    const int n = blockIdx.y;
    const MixItem it = A.items[n];
    const TrainWin o = A.objs[n];
    ti_stats_body(MixSrc{A, it, o}, o, it, A.lsum + n, s_part);
}

// the body of k_train_crops with the frame, the sources, mean and std of the ITEM
__global__ __launch_bounds__(TI_THREADS) void k_train_crops_mixed(const MixParams A)
{
    __shared__ uint8_t s_src[3 * TI_SRC_PIXELS];
    __shared__ uint8_t s_rows[3 * TI_PLANE_BYTES];
    const int n = blockIdx.z, kind = blockIdx.y, tid = threadIdx.x;   // kind 0: image, 1: mask, 2: ignore
    const int S = kind == 0 ? A.Si : A.Sm;
    const int r0 = blockIdx.x * TI_BAND;
    if (r0 >= S) return;
    const TrainWin o = A.objs[n];
    const MixItem it = A.items[n];
    float* out = kind == 0 ? A.images + (size_t)n * 3 * S * S : (kind == 1 ? A.masks : A.ignores) + (size_t)n * S * S;
    if (kind != 0 && (kind == 1 ? it.mask_kind : it.ignore_kind) == 0) {   // no source: the plane is 0.0, with no fill value
        const int r1 = min(r0 + TI_BAND, S);
        for (int i = tid; i < (r1 - r0) * S; i += TI_THREADS) out[(size_t)r0 * S + i] = 0.f;
        return;
    }
    ti_crops_body(MixSrc{A, it, o}, o, it, A.bounds, A.kk8, A.lsum + n, kind, S, r0, out, s_src, s_rows);
}

}  // namespace sdn

using namespace sdn;

SDN_API int sdn_train_crops_mixed(const int32_t* rois_host, const int32_t* objs_host, const int32_t* objs, const int32_t* items_host,
                                  const int32_t* items, int B, const int32_t* bounds, int n_bounds, const int32_t* kk8, int n_kk8,
                                  const uint8_t* nearer, int n_nearer, int image_size, int mask_size, void* workspace, float* images,
                                  float* masks, float* ignores, sdnStream stream)
{
    if (!rois_host || !objs_host || !objs || !items_host || !items || !bounds || !kk8 || !workspace || !images ||
        (n_nearer > 0 && !nearer) || (!masks) != (!ignores))
        return fail(SDN_EINVAL, "sdn_train_crops_mixed: null pointer");
    if ((reinterpret_cast<uintptr_t>(workspace) & 7) || (reinterpret_cast<uintptr_t>(items) & 7))
        return fail(SDN_EINVAL, "sdn_train_crops_mixed: the workspace and the item table must be aligned to 8 bytes");
    static_assert(sizeof(TrainWin) == MX_OBJ_INTS * sizeof(int32_t), "object table row");
    MixSizes z;
    z.B = B; z.n_bounds = n_bounds; z.n_kk8 = n_kk8; z.n_nearer = n_nearer; z.image_size = image_size; z.mask_size = mask_size;
    z.maps = masks != nullptr;
    long scon = 0;
    char why[384];
    if (mx_validate(rois_host, objs_host, items_host, z, &scon, why, sizeof(why))) return fail(SDN_EINVAL, "sdn_train_crops_mixed: %s", why);
    MixParams A;
    A.objs = reinterpret_cast<const TrainWin*>(objs);
    A.items = reinterpret_cast<const MixItem*>(items);
    A.bounds = bounds; A.kk8 = kk8; A.nearer = nearer;
    A.lsum = static_cast<unsigned long long*>(workspace);
    A.B = B; A.Si = image_size; A.Sm = mask_size;
    A.images = images; A.masks = masks; A.ignores = ignores;
    hipStream_t st = (hipStream_t)stream;
    if (scon) {
        if (hipMemsetAsync(workspace, 0, (size_t)B * sizeof(unsigned long long), st) != hipSuccess)
            return fail(SDN_ELAUNCH, "sdn_train_crops_mixed: clearing the sums failed");
        hipLaunchKernelGGL(k_train_stats_mixed, dim3(cdiv(scon * scon, TI_STAT_PIXELS), (unsigned)B), dim3(TI_THREADS), 0, st, A);
        if (int rc = check_launch("k_train_stats_mixed")) return rc;
    }
    const int Smax = z.maps ? (image_size > mask_size ? image_size : mask_size) : image_size;
    hipLaunchKernelGGL(k_train_crops_mixed, dim3(cdiv(Smax, TI_BAND), z.maps ? 3 : 1, (unsigned)B), dim3(TI_THREADS), 0, st, A);
    return check_launch("k_train_crops_mixed");
}
