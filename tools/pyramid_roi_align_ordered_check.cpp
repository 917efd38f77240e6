// Host walk over what the ordered backward of the pyramid RoIAlign adds to 3d-sdn_amd/csrc/pyramid_roi_align_check.h:
//   - the workspace size: whole 16-byte pieces, one record per box, R = 0 needs none, R < 0 and a NULL answer are refused;
//   - the grid: for many (C, H[4], W[4]) the workgroups of the four levels, laid out P5 first as the launch lays them out, are
//     decoded back into (level, tile, chunk) the way the kernel decodes them, and their tiles and channel chunks cover every element
//     of every level exactly once, none outside it; the padding floats of a level are fewer than four;
//   - the ordered validator: valid calls, everything the plain backward's validator refuses, and the workspace's own reasons.
// Host code only; build and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I3d-sdn_amd/csrc
//       tools/pyramid_roi_align_ordered_check.cpp -o /tmp/pyramid_roi_align_ordered_check && /tmp/pyramid_roi_align_ordered_check
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "pyramid_roi_align_check.h"

using namespace sdn;

static int failures = 0;

static void expect(bool ok, const char* what)
{
    if (!ok) {
        if (failures < 20) std::printf("FAIL: %s\n", what);
        failures++;
    }
}

static bool refused(int rc, const char* msg, const char* reason)
{
    return rc == 1 && std::strstr(msg, reason) != nullptr;
}

static void walk_workspace()
{
    char msg[256];
    size_t n = 77;
    const int sizes[6] = {0, 1, 5, 200, 1000, std::numeric_limits<int>::max()};
    for (int R : sizes) {
        expect(pra_ordered_workspace_bytes(R, &n, msg, sizeof(msg)) == 0 && n == (size_t)R * PRA_RECORD_BYTES && n % 16 == 0, "one record per box");
    }
    expect(PRA_RECORD_BYTES >= 5 * (int)sizeof(int) && PRA_RECORD_BYTES <= 48, "a record holds five ints and stays within a few dozen bytes");
    expect(refused(pra_ordered_workspace_bytes(-1, &n, msg, sizeof(msg)), msg, "bad sizes: R -1"), "R < 0");
    expect(refused(pra_ordered_workspace_bytes(5, nullptr, msg, sizeof(msg)), msg, "bytes is NULL"), "bytes NULL");
}

// the launch's layout of the grid (sdn_pyramid_roi_align_bwd_ordered) and the kernel's decoding of a workgroup index, on real memory
static void walk_grid(int C, const int* H, const int* W)
{
    char msg[256];
    size_t off[PRA_LEVELS], total = 0;
    if (pra_grad_layout(C, H, W, off, &total, msg, sizeof(msg))) {
        expect(false, "a valid layout");
        return;
    }
    const int chunks = pra_chunks(C);
    int start[PRA_LEVELS], blocks = 0;
    for (int k = 0; k < PRA_LEVELS; k++) {
        const int l = PRA_LEVELS - 1 - k;
        start[k] = blocks;
        blocks += pra_tiles(H[l]) * pra_tiles(W[l]) * chunks;
    }
    bool ok = (long long)blocks == pra_ordered_blocks(C, H, W);
    std::vector<unsigned char> buf(total, 0);
    for (int b = 0; b < blocks && ok; b++) {
        const int k = (b >= start[1]) + (b >= start[2]) + (b >= start[3]);
        const int l = PRA_LEVELS - 1 - k, idx = b - start[k];
        const int tiles_x = pra_tiles(W[l]), tiles = tiles_x * pra_tiles(H[l]);
        const int chunk = idx / tiles, tile = idx - chunk * tiles;
        const int ty0 = tile / tiles_x * PRA_TILE, tx0 = (tile - tile / tiles_x * tiles_x) * PRA_TILE;
        const int c0 = chunk * PRA_CHANNELS, nc = (C - c0 < PRA_CHANNELS ? C - c0 : PRA_CHANNELS);
        ok = chunk < chunks && ty0 < H[l] && tx0 < W[l] && nc >= 1;
        const int waves = PRA_THREADS / 64;
        for (int tid = 0; tid < PRA_THREADS && ok; tid++) {
            const int lane = tid & 63, wave = tid >> 6;
            const int row = ty0 + lane / PRA_TILE, col = tx0 + lane % PRA_TILE;
            const int mine = (nc - wave + waves - 1) / waves;
            ok = mine >= 0 && mine <= PRA_CHANNELS / waves;
            if (row >= H[l] || col >= W[l]) continue;
            for (int i = 0; i < mine && ok; i++) {
                const int c = c0 + wave + i * waves;
                ok = c < c0 + nc && c < C;
                if (ok) buf[off[l] + ((size_t)c * H[l] + row) * W[l] + col] += 1;
            }
        }
        const size_t used = (size_t)C * H[l] * W[l], pad = (PRA_ALIGN_FLOATS - used % PRA_ALIGN_FLOATS) % PRA_ALIGN_FLOATS;
        if (idx == 0)
            for (size_t t = 0; t < pad && ok; t++) buf[off[l] + used + t] += 1;   // the level's first workgroup writes its padding
    }
    for (size_t i = 0; i < buf.size() && ok; i++) ok = buf[i] == 1;
    expect(ok, "tiles, chunks and padding cover the gradient buffer exactly once");
}

static void walk_validator()
{
    char msg[256];
    const int H[4] = {24, 12, 6, 3}, W[4] = {20, 10, 5, 3};
    float store[8] = {};
    alignas(16) float g16[4] = {};
    alignas(16) unsigned char ws[5 * PRA_RECORD_BYTES + 16] = {};
    const float area = 1048576.0f;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const size_t need = 5 * (size_t)PRA_RECORD_BYTES;
    expect(pra_validate_bwd_ordered(store, store, H, W, 5, 67, 14, area, g16, ws, need, msg, sizeof(msg)) == 0, "a valid call");
    expect(pra_validate_bwd_ordered(store, store, H, W, 5, 67, 14, area, g16, ws, need + 16, msg, sizeof(msg)) == 0, "a larger workspace");
    expect(pra_validate_bwd_ordered(nullptr, nullptr, H, W, 0, 3, 7, area, g16, nullptr, 0, msg, sizeof(msg)) == 0, "R = 0 needs no workspace");
    expect(refused(pra_validate_bwd_ordered(nullptr, nullptr, H, W, 0, 3, 7, area, nullptr, nullptr, 0, msg, sizeof(msg)), msg, "grad_maps is NULL"),
           "R = 0 still has a buffer to write");
    // the workspace's own reasons
    expect(refused(pra_validate_bwd_ordered(store, store, H, W, 5, 3, 7, area, g16, nullptr, need, msg, sizeof(msg)), msg, "workspace is NULL with R > 0"), "workspace NULL");
    for (int shift : {1, 2, 4, 8}) {
        expect(refused(pra_validate_bwd_ordered(store, store, H, W, 5, 3, 7, area, g16, ws + shift, need, msg, sizeof(msg)), msg, "workspace must be aligned to 16"),
               "workspace misaligned");
    }
    expect(refused(pra_validate_bwd_ordered(store, store, H, W, 5, 3, 7, area, g16, ws, need - 1, msg, sizeof(msg)), msg, "159 bytes; 160 are needed for 5 boxes"),
           "workspace one byte short");
    expect(refused(pra_validate_bwd_ordered(store, store, H, W, 5, 3, 7, area, g16, ws, 0, msg, sizeof(msg)), msg, "workspace of 0 bytes"), "workspace of no bytes");
    expect(pra_validate_bwd_ordered(store, store, H, W, std::numeric_limits<int>::max(), 3, 7, area, g16, ws, (size_t)std::numeric_limits<int>::max() * PRA_RECORD_BYTES,
                                    msg, sizeof(msg)) == 0, "the largest R: its byte count does not overflow");
    // everything the plain backward's validator refuses
    expect(refused(pra_validate_bwd_ordered(store, store, H, W, -1, 3, 7, area, g16, ws, need, msg, sizeof(msg)), msg, "bad sizes: R -1"), "R < 0");
    expect(refused(pra_validate_bwd_ordered(store, store, H, W, 5, 0, 7, area, g16, ws, need, msg, sizeof(msg)), msg, "bad sizes: C 0"), "C = 0");
    expect(refused(pra_validate_bwd_ordered(store, store, nullptr, W, 5, 3, 7, area, g16, ws, need, msg, sizeof(msg)), msg, "H or W is NULL"), "H NULL");
    expect(refused(pra_validate_bwd_ordered(store, store, H, nullptr, 5, 3, 7, area, g16, ws, need, msg, sizeof(msg)), msg, "H or W is NULL"), "W NULL");
    for (int l = 0; l < 4; l++) {
        int h[4] = {24, 12, 6, 3}, w[4] = {20, 10, 5, 3};
        h[l] = 0;
        expect(refused(pra_validate_bwd_ordered(store, store, h, w, 5, 3, 7, area, g16, ws, need, msg, sizeof(msg)), msg, "bad sizes: level P"), "H = 0");
        h[l] = 65536;
        w[l] = 32768;                                                       // H * W = 2^31
        expect(refused(pra_validate_bwd_ordered(store, store, h, w, 5, 1, 7, area, g16, ws, need, msg, sizeof(msg)), msg, "below 2^31"), "H * W = 2^31");
        h[l] = 0x7fffffff;
        w[l] = 0x7fffffff;                                                  // the checks themselves must not overflow
        expect(refused(pra_validate_bwd_ordered(store, store, h, w, 5, 0x7fffffff, 7, area, g16, ws, need, msg, sizeof(msg)), msg, "below 2^31"), "huge sizes");
        // the largest maps that pass: one row (or column) of 2^31 - 1 pixels, a tile count that the grid's int still holds
        h[l] = 1;
        w[l] = 0x7fffffff;
        expect(pra_validate_bwd_ordered(store, store, h, w, 5, 1, 7, area, g16, ws, need, msg, sizeof(msg)) == 0 && pra_tiles(w[l]) == (1 << 28), "a row of 2^31 - 1 pixels");
        h[l] = 0x7fffffff;
        w[l] = 1;
        expect(pra_validate_bwd_ordered(store, store, h, w, 5, 1, 7, area, g16, ws, need, msg, sizeof(msg)) == 0, "a column of 2^31 - 1 pixels");
    }
    const int wide[4] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff}, one[4] = {1, 1, 1, 1};
    expect(pra_ordered_blocks(1, one, wide) == 4ll << 28 && pra_ordered_blocks(1, one, wide) <= std::numeric_limits<int>::max(), "the largest grid is 2^30 workgroups");
    expect(pra_validate_bwd_ordered(store, store, one, wide, 5, 1, 7, area, g16, ws, need, msg, sizeof(msg)) == 0, "four levels of 2^31 - 1 pixels");
    expect(pra_tiles(1) == 1 && pra_tiles(8) == 1 && pra_tiles(9) == 2 && pra_tiles(16) == 2 && pra_tiles(17) == 3, "tiles of eight pixels");
    expect(refused(pra_validate_bwd_ordered(store, store, H, W, 5, 3, 0, area, g16, ws, need, msg, sizeof(msg)), msg, "pool 0; 1 to 32"), "pool 0");
    expect(refused(pra_validate_bwd_ordered(store, store, H, W, 5, 3, 33, area, g16, ws, need, msg, sizeof(msg)), msg, "pool 33; 1 to 32"), "pool 33");
    expect(pra_validate_bwd_ordered(store, store, H, W, 5, 3, 32, area, g16, ws, need, msg, sizeof(msg)) == 0, "pool 32");
    const float bad_area[5] = {0.0f, -1.0f, inf, -inf, nan};
    for (float a : bad_area)
        expect(refused(pra_validate_bwd_ordered(store, store, H, W, 5, 3, 7, a, g16, ws, need, msg, sizeof(msg)), msg, "must be finite and positive"), "image_area");
    expect(refused(pra_validate_bwd_ordered(store, store, one, one, 5, 3000000, 32, area, g16, ws, need, msg, sizeof(msg)), msg, "C * pool * pool"), "C * pool^2 = 3e9");
    expect(refused(pra_validate_bwd_ordered(store, store, one, one, 0x7fffffff, 2000000, 7, area, g16, ws, need, msg, sizeof(msg)), msg, "workgroups"), "R * chunks");
    expect(refused(pra_validate_bwd_ordered(nullptr, store, H, W, 5, 3, 7, area, g16, ws, need, msg, sizeof(msg)), msg, "grads or boxes is NULL"), "grads NULL");
    expect(refused(pra_validate_bwd_ordered(store, nullptr, H, W, 5, 3, 7, area, g16, ws, need, msg, sizeof(msg)), msg, "grads or boxes is NULL"), "boxes NULL");
    expect(refused(pra_validate_bwd_ordered(reinterpret_cast<const unsigned char*>(store) + 2, store, H, W, 5, 3, 7, area, g16, ws, need, msg, sizeof(msg)), msg, "aligned to 4"),
           "grads misaligned");
    expect(refused(pra_validate_bwd_ordered(store, store, H, W, 5, 3, 7, area, nullptr, ws, need, msg, sizeof(msg)), msg, "grad_maps is NULL"), "grad_maps NULL");
    expect(refused(pra_validate_bwd_ordered(store, store, H, W, 5, 3, 7, area, g16 + 1, ws, need, msg, sizeof(msg)), msg, "aligned to 16"), "grad_maps misaligned");
}

int main()
{
    const int shapes[7][8] = {{24, 12, 6, 3, 20, 10, 5, 3}, {1, 12, 6, 1, 20, 1, 5, 1}, {1, 1, 1, 1, 1, 1, 1, 1}, {7, 3, 5, 2, 3, 3, 1, 9},
                              {37, 19, 9, 5, 41, 21, 11, 5}, {8, 16, 9, 17, 16, 8, 17, 9},   {64, 32, 16, 8, 64, 32, 16, 8}};
    int grids = 0;
    for (const auto& s : shapes)
        for (int C : {1, 2, 3, 4, 5, 63, 64, 65, 67, 130}) {
            walk_grid(C, s, s + 4);
            grids++;
        }
    walk_workspace();
    walk_validator();
    std::printf("pyramid_roi_align_ordered_check: %d grids, the workspace size, the ordered validator: %d failures\n", grids, failures);
    return failures ? 1 : 0;
}
