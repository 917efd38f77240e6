// Host walk over the index arithmetic and the validators of the Mask R-CNN training losses (3d-sdn_amd/csrc/mrcnn_loss_check.h):
//   - for every anchor count 1 .. 6000 and a few large ones: the quads of (chunk, step, lane) tile the anchors exactly once and in
//     anchor order, the last chunk is not empty; the partials of all workgroups, the table of the first pass, the head of `saved`,
//     the log-sum-exps and the prefixes lie inside their buffers, aligned, and share no byte;
//   - the ordered rank of the positive anchors as the two passes form it -- a table of the chunks' positives, each chunk re-adding
//     the entries before it, a prefix over the lanes of a step -- against a plain count, on seeded match vectors with values
//     outside {-1, 0, 1} among them;
//   - the validators: valid calls, and for every reason they name a call that must be refused with that reason.
// Host code only; build and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I3d-sdn_amd/csrc tools/mrcnn_loss_check.cpp \
//       -o /tmp/mrcnn_loss_check && /tmp/mrcnn_loss_check
#include <cstdio>
#include <cstring>
#include <vector>

#include "mrcnn_loss_check.h"

using namespace sdn;

static int failures = 0;

static void expect(bool ok, const char* what)
{
    if (!ok) {
        if (failures < 20) std::printf("FAIL: %s\n", what);
        failures++;
    }
}

static void walk_anchors(long A, int R)
{
    const int chunks = mrl_chunks(A);
    bool ok = chunks >= 1 && (long)(chunks - 1) * MRL_CHUNK < A && (long)chunks * MRL_CHUNK >= A;
    long next = 0;
    for (int c = 0; c < chunks && ok; c++)
        for (int s = 0; s < MRL_STEPS && ok; s++)
            for (int l = 0; l < MRL_THREADS && ok; l++) {
                ok = mrl_quad_first(c, s, l) == next;
                next += MRL_QUAD;
            }
    ok = ok && next >= A && next - A < MRL_CHUNK;
    // the buffers: real memory, so that ASan sees a record that leaves it
    const long nblk = mrl_blocks(A, R);
    const size_t wbytes = mrl_workspace_bytes(A, R), sbytes = mrl_saved_bytes(A, R);
    std::vector<unsigned char> work(wbytes, 0), saved(sbytes, 0);
    ok = ok && nblk == (long)chunks + R && (wbytes & 7) == 0 && (sbytes & 15) == 0;
    for (long g = 0; g < nblk && ok; g++) {
        const size_t s = mrl_sum_at(g), n = mrl_cnt_at(nblk, g);
        ok = (s & 7) == 0 && (n & 3) == 0 && s + 24 <= mrl_cnt_at(nblk, 0) && n + 16 <= mrl_table_at(nblk);
        for (size_t i = 0; i < 24 && ok; i++) work[s + i] += 1;
        for (size_t i = 0; i < 16 && ok; i++) work[n + i] += 1;
    }
    for (int c = 0; c < chunks && ok; c++) {
        const size_t t = mrl_table_at(nblk) + (size_t)c * 4, p = mrl_prefix_at(R, c);
        ok = (t & 3) == 0 && t + 4 <= wbytes && (p & 3) == 0 && p + 4 <= sbytes;
        for (size_t i = 0; i < 4 && ok; i++) {
            work[t + i] += 1;
            saved[p + i] += 1;
        }
    }
    for (int r = 0; r < R && ok; r++) {
        const size_t l = mrl_lse_at(r);
        ok = (l & 7) == 0 && l >= (size_t)MRL_SAVED_HEAD && l + 8 <= mrl_prefix_at(R, 0);
        for (size_t i = 0; i < 8 && ok; i++) saved[l + i] += 1;
    }
    for (size_t i = 0; i < wbytes && ok; i++) ok = work[i] <= 1;
    for (size_t i = MRL_SAVED_HEAD; i < sbytes && ok; i++) ok = saved[i] <= 1;
    if (!ok) {
        if (failures < 20) std::printf("A %ld, R %d: %d chunks, %zu + %zu bytes  FAIL\n", A, R, chunks, wbytes, sbytes);
        failures++;
    }
}

static unsigned long long rng_state = 88172645463325252ull;

static unsigned rng()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 11);
}

// the ranks as the kernels form them against a running count
static void walk_ranks(long A, unsigned positive_in)
{
    std::vector<long long> match((size_t)A);
    const long long values[6] = {1, -1, 0, 2, -2, (long long)1 << 40};
    for (long a = 0; a < A; a++) match[(size_t)a] = rng() % positive_in == 0 ? 1 : values[1 + rng() % 5];
    match[0] = 1;
    match[(size_t)A - 1] = 1;
    const int chunks = mrl_chunks(A);
    std::vector<int> table((size_t)chunks, 0), rank((size_t)A, -1);
    auto kind_at = [&](long a) { return a < A ? mrl_match_kind(match[(size_t)a]) : 0; };
    for (int c = 0; c < chunks; c++)   // first pass
        for (int s = 0; s < MRL_STEPS; s++)
            for (int l = 0; l < MRL_THREADS; l++)
                for (int e = 0; e < MRL_QUAD; e++) table[(size_t)c] += kind_at(mrl_quad_first(c, s, l) + e) == 1;
    for (int c = 0; c < chunks; c++) {   // second pass, every chunk on its own
        int before = 0;
        for (int i = 0; i < c; i++) before += table[(size_t)i];
        for (int s = 0; s < MRL_STEPS; s++) {
            int per_lane[MRL_THREADS], total = 0;
            for (int l = 0; l < MRL_THREADS; l++) {
                per_lane[l] = 0;
                for (int e = 0; e < MRL_QUAD; e++) per_lane[l] += kind_at(mrl_quad_first(c, s, l) + e) == 1;
            }
            for (int l = 0; l < MRL_THREADS; l++) {
                int r = before + total;
                total += per_lane[l];
                for (int e = 0; e < MRL_QUAD; e++) {
                    const long a = mrl_quad_first(c, s, l) + e;
                    if (kind_at(a) == 1) rank[(size_t)a] = r++;
                }
            }
            before += total;
        }
    }
    int count = 0;
    bool ok = true;
    for (long a = 0; a < A && ok; a++) {
        const int k = mrl_match_kind(match[(size_t)a]);
        ok = k == (match[(size_t)a] == 1 ? 1 : match[(size_t)a] == -1 ? -1 : match[(size_t)a] == 0 ? 0 : 2);
        if (k == 1) ok = ok && rank[(size_t)a] == count++;
        else ok = ok && rank[(size_t)a] == -1;
    }
    if (!ok) {
        if (failures < 20) std::printf("ranks of %ld anchors, one positive in %u  FAIL\n", A, positive_in);
        failures++;
    }
}

static bool refused(int rc, const char* msg, const char* reason)
{
    return rc == 1 && std::strstr(msg, reason) != nullptr;
}

int main()
{
    for (long A = 1; A <= 6000; A++) walk_anchors(A, (int)(A % 5));
    for (long A : {261888L, 65536L, 65537L, (long)MRL_MAX_ANCHORS - 1, (long)MRL_MAX_ANCHORS}) walk_anchors(A, 200);
    for (long A : {1L, 3L, 4L, 5L, 255L, 256L, 257L, 1023L, 1024L, 1025L, 2048L, 5003L, 261888L})
        for (unsigned every : {1u, 2u, 7u, 300u}) walk_ranks(A, every);

    expect(mrl_roi_kind(0, 3) == 0 && mrl_roi_kind(2, 3) == 1 && mrl_roi_kind(3, 3) == -1 && mrl_roi_kind(-1, 3) == -1 &&
               mrl_roi_kind((long long)1 << 32, 3) == -1,
           "the kinds of a class id");

    char msg[256];
    alignas(16) static char mem[64];
    const void* p = mem;
    const MrlInputs in = {p, 0, p, p, p, p, 1, p, p, p, p, p};
    const void* const all[5] = {p, p, p, p, p};
    const void* const none[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const void* const rpn_only[5] = {p, p, nullptr, nullptr, nullptr};
    const size_t wb = mrl_workspace_bytes(5003, 13), sb = mrl_saved_bytes(5003, 13);
    // valid calls
    expect(mrl_validate_sizes(1, 261888, 256, 200, 3, 28, 28, msg, sizeof(msg)) == 0, "the reference's sizes");
    expect(mrl_validate_sizes(1, 1, 1, 0, 0, 0, 0, msg, sizeof(msg)) == 0, "one anchor, no RoI");
    expect(mrl_validate_sizes(1, MRL_MAX_ANCHORS, 1, 1, 128, 1, 1, msg, sizeof(msg)) == 0, "the limits");
    expect(mrl_validate_fwd(in, 1, 5003, 64, 13, 3, 28, 28, p, wb, p, sb, p, p, msg, sizeof(msg)) == 0, "a valid forward call");
    expect(mrl_validate_bwd(in, 1, 5003, 64, 13, 3, 28, 28, p, sb, p, all, msg, sizeof(msg)) == 0, "a valid backward call");
    MrlInputs rpn = in;
    rpn.target_class_ids = rpn.mrcnn_class_logits = rpn.target_deltas = rpn.mrcnn_bbox = rpn.target_mask = rpn.mrcnn_mask = nullptr;
    expect(mrl_validate_fwd(rpn, 1, 777, 8, 0, 0, 0, 0, p, mrl_workspace_bytes(777, 0), p, mrl_saved_bytes(777, 0), p, p, msg, sizeof(msg)) == 0,
           "R = 0 without head tensors");
    expect(mrl_validate_bwd(rpn, 1, 777, 8, 0, 0, 0, 0, p, mrl_saved_bytes(777, 0), p, rpn_only, msg, sizeof(msg)) == 0, "R = 0 backward");
    // refusals
    expect(refused(mrl_validate_sizes(2, 100, 8, 1, 3, 5, 7, msg, sizeof(msg)), msg, "model.py:1053"), "batch 2");
    expect(refused(mrl_validate_sizes(0, 100, 8, 1, 3, 5, 7, msg, sizeof(msg)), msg, "batch 0"), "batch 0");
    expect(refused(mrl_validate_sizes(1, 0, 8, 1, 3, 5, 7, msg, sizeof(msg)), msg, "bad sizes"), "A = 0");
    expect(refused(mrl_validate_sizes(1, 100, 0, 1, 3, 5, 7, msg, sizeof(msg)), msg, "bad sizes"), "T = 0");
    expect(refused(mrl_validate_sizes(1, MRL_MAX_ANCHORS + 1, 8, 1, 3, 5, 7, msg, sizeof(msg)), msg, "anchors"), "too many anchors");
    expect(refused(mrl_validate_sizes(1, 100, 2147483647, 1, 3, 5, 7, msg, sizeof(msg)), msg, "below 2^31"), "T * 4 overflows");
    expect(refused(mrl_validate_sizes(1, 100, 8, -1, 3, 5, 7, msg, sizeof(msg)), msg, "bad sizes"), "R < 0");
    expect(refused(mrl_validate_sizes(1, 100, 8, 1, 1, 5, 7, msg, sizeof(msg)), msg, "1 classes; 2 to 128"), "C = 1");
    expect(refused(mrl_validate_sizes(1, 100, 8, 1, 129, 5, 7, msg, sizeof(msg)), msg, "129 classes; 2 to 128"), "C = 129");
    expect(refused(mrl_validate_sizes(1, 100, 8, 1, 3, 0, 7, msg, sizeof(msg)), msg, "bad sizes"), "h = 0");
    expect(refused(mrl_validate_sizes(1, 100, 8, 4, 128, 2048, 2048, msg, sizeof(msg)), msg, "below 2^31"), "exactly 2^31");
    expect(refused(mrl_validate_sizes(1, 100, 8, 2147483647, 128, 2147483647, 2147483647, msg, sizeof(msg)), msg, "below 2^31"),
           "factors near 2^31");
    MrlInputs bad = in;
    bad.rpn_match = nullptr;
    expect(refused(mrl_validate_fwd(bad, 1, 100, 8, 1, 3, 5, 7, p, 1 << 20, p, 1 << 20, p, p, msg, sizeof(msg)), msg, "rpn_match is NULL"), "null match");
    bad = in;
    bad.rpn_pred_bbox = nullptr;
    expect(refused(mrl_validate_fwd(bad, 1, 100, 8, 1, 3, 5, 7, p, 1 << 20, p, 1 << 20, p, p, msg, sizeof(msg)), msg, "is NULL"), "null pred");
    bad = in;
    bad.mrcnn_mask = nullptr;
    expect(refused(mrl_validate_fwd(bad, 1, 100, 8, 1, 3, 5, 7, p, 1 << 20, p, 1 << 20, p, p, msg, sizeof(msg)), msg, "head tensor is NULL"), "null mask");
    bad = in;
    bad.match_i64 = 2;
    expect(refused(mrl_validate_fwd(bad, 1, 100, 8, 1, 3, 5, 7, p, 1 << 20, p, 1 << 20, p, p, msg, sizeof(msg)), msg, "type flag"), "a bad type flag");
    bad = in;
    bad.target_class_ids = mem + 4;   // int64 ids
    expect(refused(mrl_validate_fwd(bad, 1, 100, 8, 1, 3, 5, 7, p, 1 << 20, p, 1 << 20, p, p, msg, sizeof(msg)), msg, "element size"), "misaligned ids");
    bad = in;
    bad.rpn_class_logits = mem + 2;
    expect(refused(mrl_validate_fwd(bad, 1, 100, 8, 1, 3, 5, 7, p, 1 << 20, p, 1 << 20, p, p, msg, sizeof(msg)), msg, "aligned to 4"), "misaligned logits");
    expect(refused(mrl_validate_fwd(in, 1, 100, 8, 1, 3, 5, 7, p, 1 << 20, p, 1 << 20, nullptr, p, msg, sizeof(msg)), msg, "is NULL"), "null out");
    expect(refused(mrl_validate_fwd(in, 1, 100, 8, 1, 3, 5, 7, p, 1 << 20, p, 1 << 20, p, mem + 4, msg, sizeof(msg)), msg, "aligned to 8"), "misaligned counts");
    expect(refused(mrl_validate_fwd(in, 1, 5003, 64, 13, 3, 28, 28, p, wb - 1, p, sb, p, p, msg, sizeof(msg)), msg, "workspace of"), "a short workspace");
    expect(refused(mrl_validate_fwd(in, 1, 5003, 64, 13, 3, 28, 28, p, wb, p, sb - 1, p, p, msg, sizeof(msg)), msg, "saved of"), "a short saved");
    expect(refused(mrl_validate_bwd(in, 1, 100, 8, 1, 3, 5, 7, p, 1 << 20, p, none, msg, sizeof(msg)), msg, "no gradient"), "bwd: no gradient");
    expect(refused(mrl_validate_bwd(rpn, 1, 100, 8, 0, 0, 0, 0, p, 1 << 20, p, all, msg, sizeof(msg)), msg, "R = 0"), "bwd: head gradient without RoIs");
    expect(refused(mrl_validate_bwd(in, 1, 100, 8, 1, 3, 5, 7, p, 1 << 20, nullptr, all, msg, sizeof(msg)), msg, "is NULL"), "bwd: null grad_out");
    expect(refused(mrl_validate_bwd(in, 2, 100, 8, 1, 3, 5, 7, p, 1 << 20, p, all, msg, sizeof(msg)), msg, "model.py:1053"), "bwd: batch 2");
    // a message longer than its buffer is cut, not overrun
    char tiny[8];
    expect(mrl_validate_sizes(1, 100, 8, 1, 129, 5, 7, tiny, sizeof(tiny)) == 1 && std::strlen(tiny) == 7, "a short message buffer");

    std::printf("mrcnn_loss_check: 6005 anchor counts, 52 rank walks, validators: %d failures\n", failures);
    return failures ? 1 : 0;
}
