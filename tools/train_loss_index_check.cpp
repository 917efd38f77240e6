// Host walk over the index arithmetic of sdn_train_losses_* (3d-sdn_amd/csrc/train_loss_index.h): for every (R, S) below, every
// pixel of the R x R rendered mask is visited through the kernels' own block / chunk / thread decomposition, every address the
// scalar and the 16-byte paths would form is written down in real S x S and R x R arrays (so an address sanitizer sees an
// overrun), checked against [0, S), and the weighted sum is compared with the padded-copy formulation of the reference.
// Host code only; build and run on the CPU, e.g.
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -I3d-sdn_amd/csrc \
//         tools/train_loss_index_check.cpp -o /tmp/train_loss_index_check && /tmp/train_loss_index_check
// (or any C++17 compiler: g++ -fsanitize=address,undefined -I3d-sdn_amd/csrc ...).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "train_loss_index.h"

using namespace sdn;

static int failures = 0;
#define EXPECT(c, ...)                \
    do {                              \
        if (!(c)) {                   \
            std::printf(__VA_ARGS__); \
            std::printf("\n");        \
            failures++;               \
        }                             \
    } while (0)

static double check_pair(int R, int S)
{
    const int p = (R - S) / 2;
    std::vector<float> render((size_t)R * R), mask((size_t)S * S), ign((size_t)S * S);
    for (size_t i = 0; i < render.size(); i++) render[i] = (float)((i * 7919u) % 101) / 101.f;
    for (size_t i = 0; i < mask.size(); i++) mask[i] = (float)((i * 31u) % 256) / 255.f;
    for (size_t i = 0; i < ign.size(); i++) ign[i] = (float)((i * 17u + 3) % 255) / 255.f;
    std::vector<int> seen((size_t)R * R, 0);

    // the padded copies of the reference: F.pad(mask, p, 'constant', 0), F.pad(ign, p, 'replicate')
    double want = 0.0;
    for (int y = 0; y < R; y++)
        for (int x = 0; x < R; x++) {
            const int u = y - p, v = x - p;
            const float m = (u >= 0 && u < S && v >= 0 && v < S) ? mask[(size_t)u * S + v] : 0.f;
            const int cu = u < 0 ? 0 : (u > S - 1 ? S - 1 : u), cv = v < 0 ? 0 : (v > S - 1 ? S - 1 : v);
            const double d = (double)render[(size_t)y * R + x] - (double)m;
            want += (1.0 - (double)ign[(size_t)cu * S + cv]) * d * d;
        }

    // the kernels' decomposition: chunks of tl_rows(R) rows, TL_THREADS threads striding over the chunk
    const int rows = tl_rows(R), C = tl_chunks(R);
    EXPECT(rows >= 1 && (long)C * rows >= R && (long)(C - 1) * rows < R, "R %d: %d chunks of %d rows do not tile the rows", R, C, rows);
    const bool vr = R % 4 == 0, vs = vr && S % 4 == 0 && p % 4 == 0;
    double got = 0.0;
    for (int c = 0; c < C; c++) {
        const int y0 = c * rows, y1 = (y0 + rows < R) ? y0 + rows : R;
        for (int t = 0; t < TL_THREADS; t++) {
            if (vr) {
                const int R4 = R >> 2, n4 = (y1 - y0) * R4;
                for (int e = t; e < n4; e += TL_THREADS) {
                    const int dy = e / R4, x = (e - dy * R4) << 2, y = y0 + dy;
                    EXPECT(y >= 0 && y < R && x >= 0 && x + 3 < R, "R %d S %d: render group (%d, %d) outside", R, S, y, x);
                    const int yy = tl_clamp(y, p, S);
                    EXPECT(yy >= 0 && yy < S, "R %d S %d: ignore row %d", R, S, yy);
                    float m[4], g[4];
                    if (vs) {
                        int edge = -1;
                        const int v = tl_group(x, p, S, &edge);
                        if (v >= 0) {
                            EXPECT(v + 3 < S && v % 4 == 0, "R %d S %d: group at source column %d", R, S, v);
                            for (int k = 0; k < 4; k++) {
                                g[k] = ign[(size_t)yy * S + v + k];
                                m[k] = tl_inside(y, p, S) ? mask[(size_t)(y - p) * S + v + k] : 0.f;
                            }
                        } else {
                            EXPECT(edge == 0 || edge == S - 1, "R %d S %d: edge column %d", R, S, edge);
                            for (int k = 0; k < 4; k++) {
                                EXPECT(!tl_inside(x + k, p, S), "R %d S %d: column %d is not padding", R, S, x + k);
                                g[k] = ign[(size_t)yy * S + edge];
                                m[k] = 0.f;
                            }
                        }
                    } else {
                        for (int k = 0; k < 4; k++) {
                            const int xx = tl_clamp(x + k, p, S);
                            EXPECT(xx >= 0 && xx < S, "R %d S %d: ignore column %d", R, S, xx);
                            g[k] = ign[(size_t)yy * S + xx];
                            const bool in = tl_inside(y, p, S) && tl_inside(x + k, p, S);
                            if (in) EXPECT(y - p >= 0 && y - p < S && x + k - p >= 0 && x + k - p < S, "R %d S %d: mask (%d, %d)", R, S, y - p, x + k - p);
                            m[k] = in ? mask[(size_t)(y - p) * S + (x + k - p)] : 0.f;
                        }
                    }
                    for (int k = 0; k < 4; k++) {
                        const double d = (double)render[(size_t)y * R + x + k] - (double)m[k];
                        got += (1.0 - (double)g[k]) * d * d;
                        seen[(size_t)y * R + x + k]++;
                    }
                }
            } else {
                const int n = (y1 - y0) * R;
                for (int e = t; e < n; e += TL_THREADS) {
                    const int dy = e / R, x = e - dy * R, y = y0 + dy;
                    EXPECT(y >= 0 && y < R && x >= 0 && x < R, "R %d S %d: render (%d, %d) outside", R, S, y, x);
                    const int yy = tl_clamp(y, p, S), xx = tl_clamp(x, p, S);
                    EXPECT(yy >= 0 && yy < S && xx >= 0 && xx < S, "R %d S %d: ignore (%d, %d)", R, S, yy, xx);
                    const bool in = tl_inside(y, p, S) && tl_inside(x, p, S);
                    if (in) EXPECT(y - p >= 0 && y - p < S && x - p >= 0 && x - p < S, "R %d S %d: mask (%d, %d)", R, S, y - p, x - p);
                    const float m = in ? mask[(size_t)(y - p) * S + (x - p)] : 0.f;
                    const double d = (double)render[(size_t)y * R + x] - (double)m;
                    got += (1.0 - (double)ign[(size_t)yy * S + xx]) * d * d;
                    seen[(size_t)y * R + x]++;
                }
            }
        }
    }
    for (size_t i = 0; i < seen.size(); i++)
        if (seen[i] != 1) {
            EXPECT(false, "R %d S %d: pixel %zu visited %d times", R, S, i, seen[i]);
            break;
        }
    const double err = got > want ? got - want : want - got;
    EXPECT(err <= 1e-12 * want, "R %d S %d: sum %.17g, padded copies give %.17g", R, S, got, want);
    std::printf("R %3d S %3d p %2d  %s  %d chunk(s) of %d rows  sum %.12g\n", R, S, p, vs ? "16-byte maps" : (vr ? "16-byte render" : "scalar"), C, rows, got);
    return got;
}

int main()
{
    const int pairs[][2] = {{40, 32}, {32, 32}, {38, 32}, {48, 32}, {36, 32}, {96, 64}, {90, 64}, {384, 256}, {64, 64}, {2, 2}, {1, 1},
                            {6, 4}, {4100, 4096}, {5000, 4}};
    for (const auto& rs : pairs) check_pair(rs[0], rs[1]);
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("train_loss_index_check: ok\n");
    return 0;
}
