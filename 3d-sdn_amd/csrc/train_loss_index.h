// Index arithmetic of sdn_train_losses_* (train_loss.hip): how a pixel of the R x R rendered mask finds its pixel of the S x S
// target mask / ignore map under Transforms.pad_like (derender3d/datasets.py:29-33: (R - S) // 2 on both sides; 'constant' 0
// for the masks, 'replicate' for the ignore maps), and how an item's rows are cut into the chunks of a block.  Host and device
// share it so that a host program can walk every generated index (tools/train_loss_index_check.cpp).
#pragma once

#if defined(__HIPCC__)
#define SDN_TL_HD __host__ __device__
#else
#define SDN_TL_HD
#endif

namespace sdn {

constexpr int TL_THREADS = 256;
constexpr int TL_SPAN = 4096;   // floats of _masks per block: four 16-byte loads per thread before another block pays

// rows of the rendered mask per block, and blocks (chunks) per item
SDN_TL_HD inline int tl_rows(int R) { return R >= TL_SPAN ? 1 : TL_SPAN / R; }
SDN_TL_HD inline int tl_chunks(int R) { return (R + tl_rows(R) - 1) / tl_rows(R); }

// row / column v of the padded map lies inside the S-wide source (the masks are 0 outside)
SDN_TL_HD inline bool tl_inside(int v, int p, int S) { return v >= p && v - p < S; }
// the source row / column a padded ignore map shows at v: clamped into [0, S - 1]
SDN_TL_HD inline int tl_clamp(int v, int p, int S)
{
    const int u = v - p;
    return u < 0 ? 0 : (u >= S ? S - 1 : u);
}

// The 16-byte path over masks / ignores: x, p and S multiples of 4, so columns x .. x + 3 map to source columns x - p .. x - p + 3
// that lie inside [0, S) all four or not at all.  Returns the first source column, or -1 when the four are padding; then
// *edge is the one column the replicate padding repeats.
SDN_TL_HD inline int tl_group(int x, int p, int S, int* edge)
{
    const int v = x - p;
    if (v >= 0 && v < S) return v;
    *edge = v < 0 ? 0 : S - 1;
    return -1;
}

}  // namespace sdn
