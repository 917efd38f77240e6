// Host walk over the block arithmetic and the validators of the semantic training loss (3d-sdn_amd/csrc/segm_loss_check.h):
//   - for every plane size 1 .. 3000 and a few large ones: the chunks of an item tile its pixels exactly once, none is empty, the
//     last one ends at the plane; with h w % 4 == 0 no quad of four adjacent pixels straddles the plane's end; the partials of all
//     workgroups lie inside the scratch, 8-byte aligned, sums and counts apart;
//   - the validators: valid calls, and for every reason they name a call that must be refused with that reason (the sizes at
//     and just below 2^31, factors that would overflow a 32- or 64-bit product).
// Host code only; build and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I3d-sdn_amd/csrc tools/segm_loss_check.cpp \
//       -o /tmp/segm_loss_check && /tmp/segm_loss_check
#include <cstdio>
#include <cstring>
#include <vector>

#include "segm_loss_check.h"

using namespace sdn;

static int failures = 0;

static void expect(bool ok, const char* what)
{
    if (!ok) {
        if (failures < 20) std::printf("FAIL: %s\n", what);
        failures++;
    }
}

static void walk_plane(int B, long HW)
{
    const int chunks = sgl_chunks(HW);
    const long nblk = sgl_blocks(B, HW);
    const size_t bytes = sgl_scratch_bytes(B, HW);
    std::vector<unsigned char> scratch(bytes, 0);   // real memory: ASan sees a partial that leaves it
    long covered = 0;
    bool ok = chunks >= 1 && nblk == (long)B * chunks;
    for (int k = 0; k < chunks && ok; k++) {
        long first;
        int count;
        sgl_chunk_range(HW, k, &first, &count);
        ok = first == covered && count >= 1 && count <= SGL_PIXELS && first + count <= HW;
        if ((HW & 3) == 0) ok = ok && (count & 3) == 0;   // the 16-byte path: whole quads only
        covered += count;
    }
    ok = ok && covered == HW;
    long f;
    int c;
    sgl_chunk_range(HW, chunks, &f, &c);
    ok = ok && c == 0;
    for (long g = 0; g < nblk && ok; g++) {
        const size_t s = sgl_sum_at(g), n = sgl_cnt_at(nblk, g);
        ok = (s & 7) == 0 && (n & 3) == 0 && s + 16 <= sgl_cnt_at(nblk, 0) && n + 16 <= bytes;
        if (ok) {
            scratch[s] += 1; scratch[s + 15] += 1;
            scratch[n] += 1; scratch[n + 15] += 1;
        }
    }
    for (size_t i = 0; i < bytes && ok; i++) ok = scratch[i] <= 1;   // no two partials share a byte
    if (!ok) {
        if (failures < 20) std::printf("B %d, %ld pixels: %d chunks, %ld workgroups, %zu bytes  FAIL\n", B, HW, chunks, nblk, bytes);
        failures++;
    }
}

static bool refused(int rc, const char* msg, const char* reason)
{
    return rc == 1 && std::strstr(msg, reason) != nullptr;
}

int main()
{
    for (long HW = 1; HW <= 3000; HW++) walk_plane(HW % 3 + 1, HW);
    for (long HW : {7488L, 65536L, 65537L, 1L << 20, (1L << 20) + 3}) walk_plane(2, HW);

    char msg[256];
    alignas(16) static char mem[64];
    const void* p = mem;
    // valid calls
    expect(sgl_validate_sizes(2, 14, 48, 156, msg, sizeof(msg)) == 0, "the default size");
    expect(sgl_validate_sizes(1, 32, 1, 1, msg, sizeof(msg)) == 0, "one pixel, 32 classes");
    expect(sgl_validate_sizes(1, 1, 46340, 46340, msg, sizeof(msg)) == 0, "46340^2 < 2^31");
    expect(sgl_validate_sizes(1, 1, 1, 2147483647, msg, sizeof(msg)) == 0, "2^31 - 1 pixels");
    expect(sgl_validate_fwd(p, p, p, sgl_scratch_bytes(3, 480), p, p, p, 3, 14, 12, 40, msg, sizeof(msg)) == 0, "a valid forward call");
    expect(sgl_validate_bwd(p, nullptr, p, p, p, p, p, nullptr, 3, 14, 12, 40, msg, sizeof(msg)) == 0, "a valid backward call, one head");
    // refusals
    expect(refused(sgl_validate_sizes(2, 0, 5, 7, msg, sizeof(msg)), msg, "0 classes"), "C = 0");
    expect(refused(sgl_validate_sizes(2, 33, 5, 7, msg, sizeof(msg)), msg, "33 classes"), "C = 33");
    expect(refused(sgl_validate_sizes(0, 14, 5, 7, msg, sizeof(msg)), msg, "bad sizes"), "B = 0");
    expect(refused(sgl_validate_sizes(2, 14, -1, 7, msg, sizeof(msg)), msg, "bad sizes"), "h < 0");
    expect(refused(sgl_validate_sizes(4, 32, 4096, 4096, msg, sizeof(msg)), msg, "below 2^31"), "exactly 2^31");
    expect(refused(sgl_validate_sizes(1, 1, 65536, 32768, msg, sizeof(msg)), msg, "below 2^31"), "h w = 2^31");
    expect(refused(sgl_validate_sizes(2147483647, 32, 2147483647, 2147483647, msg, sizeof(msg)), msg, "below 2^31"), "factors near 2^31");
    expect(refused(sgl_validate_sizes(2, 1, 46341, 46341, msg, sizeof(msg)), msg, "below 2^31"), "2 * 46341^2");
    expect(refused(sgl_validate_fwd(nullptr, p, p, 1 << 20, p, p, p, 2, 14, 5, 7, msg, sizeof(msg)), msg, "scores is NULL"), "null scores");
    expect(refused(sgl_validate_fwd(p, nullptr, p, 1 << 20, p, p, p, 2, 14, 5, 7, msg, sizeof(msg)), msg, "seg_label is NULL"), "null label");
    expect(refused(sgl_validate_fwd(p, p, p, 1 << 20, p, nullptr, p, 2, 14, 5, 7, msg, sizeof(msg)), msg, "NULL"), "null out");
    expect(refused(sgl_validate_fwd(p, p, p, sgl_scratch_bytes(3, 480) - 1, p, p, p, 3, 14, 12, 40, msg, sizeof(msg)), msg, "are needed"),
           "a scratch one byte short");
    expect(refused(sgl_validate_fwd(p, mem + 4, p, 1 << 20, p, p, p, 2, 14, 5, 7, msg, sizeof(msg)), msg, "aligned to 8"), "a misaligned label");
    expect(refused(sgl_validate_fwd(p, p, mem + 2, 1 << 20, p, p, p, 2, 14, 5, 7, msg, sizeof(msg)), msg, "aligned to 8"), "a misaligned scratch");
    expect(refused(sgl_validate_bwd(p, p, nullptr, p, p, p, p, p, 2, 14, 5, 7, msg, sizeof(msg)), msg, "seg_label is NULL"), "bwd: null label");
    expect(refused(sgl_validate_bwd(p, p, p, p, p, p, nullptr, nullptr, 2, 14, 5, 7, msg, sizeof(msg)), msg, "no gradient"), "bwd: no gradient");
    expect(refused(sgl_validate_bwd(nullptr, p, p, p, p, p, p, nullptr, 2, 14, 5, 7, msg, sizeof(msg)), msg, "without scores"), "bwd: no scores");
    expect(refused(sgl_validate_bwd(p, nullptr, p, p, p, p, nullptr, p, 2, 14, 5, 7, msg, sizeof(msg)), msg, "without scores_deepsup"),
           "bwd: no deepsup scores");
    expect(refused(sgl_validate_bwd(p, p, p, p, p, p, p, p, 2, 33, 5, 7, msg, sizeof(msg)), msg, "33 classes"), "bwd: C = 33");
    // a message longer than its buffer is cut, not overrun
    char tiny[8];
    expect(sgl_validate_sizes(2, 33, 5, 7, tiny, sizeof(tiny)) == 1 && std::strlen(tiny) == 7, "a short message buffer");

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("segm_loss_check: chunk walk over 3005 plane sizes and 27 validator cases ok\n");
    return 0;
}
