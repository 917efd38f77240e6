// Host walk over the index, key, bitmap and prefix arithmetic and the validators of the textural input encoding
// (3d-sdn_amd/csrc/encode_input_check.h):
//   - the channel of an index map's value: truncation toward zero, the edges of [0, channels), NaN and Inf;
//   - the key rule inst * bs + i in fp32 (exact up to 2^24: VKITTI's 255 000 * 8 + 7), int32 and int16 (wraparound);
//   - the window: its first and last key, one key outside each end, fractions at the ends, NaN and Inf;
//   - the bitmap / prefix / rank scheme on random key sets against a sorted list, with the scan's split of the words over the
//     threads of its workgroup and the workspace layout;
//   - the validators: valid calls and one refused call per reason.
// Host code only; build and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -I3d-sdn_amd/csrc tools/encode_input_check.cpp -o /tmp/encode_input_check && /tmp/encode_input_check
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <set>
#include <vector>

#include "encode_input_check.h"

using namespace sdn;

static int failures = 0;

static void expect(bool ok, const char* what)
{
    if (!ok) {
        if (failures < 20) std::printf("FAIL: %s\n", what);
        failures++;
    }
}

static void walk_channels()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (int ch : {1, 14, 25, 256}) {
        expect(enc_channel_f32(0.f, ch) == 0 && enc_channel_f32(-0.f, ch) == 0, "0 selects plane 0");
        expect(enc_channel_f32(-0.5f, ch) == 0 && enc_channel_f32(-0.999f, ch) == 0, "a negative fraction truncates to plane 0");
        expect(enc_channel_f32(0.999f, ch) == 0, "a fraction truncates toward zero");
        expect(enc_channel_f32(-1.f, ch) == -1 && enc_channel_f32(-1e30f, ch) == -1, "negative indices are bad");
        expect(enc_channel_f32((float)ch, ch) == -1 && enc_channel_f32(1e30f, ch) == -1, "indices from `channels` on are bad");
        expect(enc_channel_f32(std::nextafterf((float)ch, 0.f), ch) == ch - 1, "the last float below `channels` is the last plane");
        expect(enc_channel_f32(nan, ch) == -1 && enc_channel_f32(inf, ch) == -1 && enc_channel_f32(-inf, ch) == -1, "NaN and Inf are bad");
        for (int v = -3; v <= ch + 2; v++) {
            const int want = (v >= 0 && v < ch) ? v : -1;
            expect(enc_channel_i32(v, ch) == want && enc_channel_f32((float)v, ch) == want, "integers select their own plane");
            if (v >= 0 && v < ch) expect(enc_channel_f32((float)v + 0.75f, ch) == v, "v + 0.75 truncates to v");
        }
        expect(enc_channel_i32(INT_MIN, ch) == -1 && enc_channel_i32(INT_MAX, ch) == -1, "the ends of int32 are bad");
    }
    expect(enc_elem_bytes(ENC_U8) == 1 && enc_elem_bytes(ENC_I16) == 2 && enc_elem_bytes(ENC_I32) == 4 && enc_elem_bytes(ENC_F32) == 4,
           "element sizes");
}

static void walk_keys()
{
    // fp32: exact while the result stays below 2^24
    for (int bs : {1, 2, 3, 4, 8})
        for (int i = 0; i < bs; i++)
            for (long v : {0L, 7L, 26L, 1000L, 26000L, 255000L}) {
                const float d = idx_disambiguate_f32((float)v, bs, i);
                expect((double)d == (double)(v * bs + i), "fp32 keys are exact below 2^24");
                const int bit = idx_bit_f32(d);
                expect(v * bs + i > IDX_KEY_MIN + IDX_BITS - 1 ? bit == -1 : bit == (int)(v * bs + i - IDX_KEY_MIN), "fp32 bit of a key");
            }
    expect(idx_bit_f32(idx_disambiguate_f32(255000.f, 8, 7)) == 2040007 - IDX_KEY_MIN, "255 000 * 8 + 7 lies inside the window");
    // int32 and int16 wrap
    expect(idx_disambiguate_i32(INT_MAX, 2, 1) == -1, "int32 wraps: (2^31 - 1) * 2 + 1 = -1");
    expect(idx_disambiguate_i32(-5, 3, 2) == -13, "int32 negative values");
    expect(idx_disambiguate_i16(20000, 4, 0) == (int16_t)14464 && idx_disambiguate_i16(20000, 4, 3) == (int16_t)14467, "int16 wraps: 20 000 * 4");
    expect(idx_disambiguate_i16(-20000, 4, 1) == (int16_t)-14463 && idx_disambiguate_i16(32767, 4, 2) == (int16_t)-2, "int16 wraps: negative, 32767");
    for (int v = -32768; v <= 32767; v += 13)
        for (int bs : {1, 2, 3, 4, 8}) {
            const int16_t d = idx_disambiguate_i16((int16_t)v, bs, bs - 1);
            const long full = (long)v * bs + bs - 1;
            const long wrapped = ((full % 65536) + 65536 + 32768) % 65536 - 32768;
            expect((long)d == wrapped, "int16 key = (v * bs + i) mod 2^16, signed");
            expect(idx_bit_i32((int32_t)d) == (int)d - IDX_KEY_MIN, "every int16 key lies inside the window");
        }
    // the window
    const int last = IDX_KEY_MIN + IDX_BITS - 1;
    expect(idx_bit_i32(IDX_KEY_MIN) == 0 && idx_bit_i32(last) == IDX_BITS - 1, "first and last key, int32");
    expect(idx_bit_i32(IDX_KEY_MIN - 1) == -1 && idx_bit_i32(last + 1) == -1 && idx_bit_i32(INT_MIN) == -1 && idx_bit_i32(INT_MAX) == -1,
           "keys outside the window, int32");
    expect(idx_bit_f32((float)IDX_KEY_MIN) == 0 && idx_bit_f32((float)last) == IDX_BITS - 1, "first and last key, fp32");
    expect(idx_bit_f32((float)IDX_KEY_MIN - 0.5f) == 0 && idx_bit_f32((float)last + 0.5f) == IDX_BITS - 1, "fractions at the ends truncate inward");
    expect(idx_bit_f32((float)(IDX_KEY_MIN - 1)) == -1 && idx_bit_f32((float)(last + 1)) == -1, "one key outside each end, fp32");
    expect(idx_bit_f32(-0.5f) == -IDX_KEY_MIN && idx_bit_f32(0.5f) == -IDX_KEY_MIN, "-0.5 and 0.5 are key 0");
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    expect(idx_bit_f32(nan) == -1 && idx_bit_f32(inf) == -1 && idx_bit_f32(-inf) == -1 && idx_bit_f32(3e38f) == -1, "NaN, Inf and huge values overflow");
    expect(idx_key_of_bit(0) == IDX_KEY_MIN && idx_key_of_bit(IDX_BITS - 1) == last, "bit back to key");
    expect(IDX_KEY_MIN % 32 == 0, "key 32 k begins a word");
}

static long ranked = 0;

// the scheme of k_inst_mark / k_inst_scan / k_inst_rank on a key set, with the scan's thread split
static void walk_scheme(const std::vector<long>& keys)
{
    std::vector<uint32_t> bitmap(IDX_WORDS, 0u);
    std::vector<int> prefix(IDX_WORDS, -1);
    for (long k : keys) {
        const int bit = idx_bit_i32((int32_t)k);
        expect(bit >= 0 && bit < IDX_BITS, "a window key has a bit");
        bitmap[bit >> 5] |= 1u << (bit & 31);
    }
    // k_inst_scan's order: wave v owns 4096 consecutive words; in step j lane l holds the four words at 4096 v + 256 j + 4 l;
    // a scan across the lanes, a running total across the steps, the waves' totals at the end
    std::vector<int> wave_total(IDX_SCAN_WAVES, 0);
    std::vector<int> local(IDX_WORDS, -1);   // set bits of the wave's words before a word
    std::vector<char> covered(IDX_WORDS, 0);
    for (int v = 0; v < IDX_SCAN_WAVES; v++) {
        int run = 0;
        for (int j = 0; j < IDX_SCAN_STEPS; j++) {
            int incl = 0;
            for (int l = 0; l < 64; l++) {
                const size_t w = (size_t)v * IDX_WAVE_WORDS + (size_t)j * 256 + (size_t)l * 4;
                int r = run + incl;   // the lane's exclusive prefix
                for (int k = 0; k < 4; k++) {
                    expect(w + k < (size_t)IDX_WORDS && !covered[w + k], "a word is scanned once");
                    covered[w + k] = 1;
                    local[w + k] = r;
                    r += idx_popc(bitmap[w + k]);
                }
                incl = r - run;
            }
            run += incl;
        }
        wave_total[v] = run;
    }
    int run = 0;
    for (int v = 0; v < IDX_SCAN_WAVES; v++) {
        for (int w = 0; w < IDX_WAVE_WORDS; w++) prefix[(size_t)v * IDX_WAVE_WORDS + w] = run + local[(size_t)v * IDX_WAVE_WORDS + w];
        run += wave_total[v];
    }
    {
        int r = 0;
        for (int w = 0; w < IDX_WORDS; w++) {
            expect(covered[w] && prefix[w] == r, "a word's prefix counts the set bits of all words before it");
            r += idx_popc(bitmap[w]);
        }
    }
    const std::set<long> unique(keys.begin(), keys.end());
    expect(run == (int)unique.size(), "K is the number of distinct keys");
    std::vector<long> ids(unique.size(), LONG_MIN);
    for (int w = 0; w < IDX_WORDS; w++)
        for (int b = 0; b < 32; b++)
            if ((bitmap[w] >> b) & 1u) {
                const int k = idx_rank(prefix[w], bitmap[w], b);
                expect(k >= 0 && k < (int)ids.size(), "an id's slot lies inside ids");
                if (k >= 0 && k < (int)ids.size()) ids[k] = idx_key_of_bit(w * 32 + b);
            }
    expect(std::equal(ids.begin(), ids.end(), unique.begin()), "ids are the distinct keys in ascending order");
    for (long k : keys) {
        const int bit = idx_bit_i32((int32_t)k);
        const int seg = idx_rank(prefix[bit >> 5], bitmap[bit >> 5], bit);
        expect(seg >= 0 && seg < (int)ids.size() && ids[seg] == k, "ids[seg] is the pixel's key");
        ranked++;
    }
}

static void walk_validators()
{
    char msg[256];
    alignas(16) static char buf[64];
    void* ok = buf;
    void* odd = buf + 2;
    const auto has = [&](const char* what) { return std::strstr(msg, what) != nullptr; };
    expect(enc_validate_maps(ok, ENC_U8, ok, ENC_I16, ok, ENC_F32, 4, 384, 1248, 14, 25, ok, ok, ok, msg, sizeof(msg)) == 0, "the full size is valid");
    expect(enc_validate_maps(ok, ENC_F32, nullptr, 0, nullptr, 0, 1, 1, 1, 1, 0, ok, nullptr, ok, msg, sizeof(msg)) == 0, "no inst, no pose is valid");
    expect(enc_validate_maps(buf + 1, ENC_U8, buf + 2, ENC_I16, ok, ENC_I32, 1, 2, 3, 256, 256, ok, ok, ok, msg, sizeof(msg)) == 0,
           "maps aligned to their element size, 256 channels");
    expect(enc_validate_maps(nullptr, ENC_U8, ok, ENC_I16, ok, ENC_F32, 1, 2, 3, 14, 25, ok, ok, ok, msg, sizeof(msg)) == 1 && has("label is NULL"), "label NULL");
    expect(enc_validate_maps(ok, ENC_U8, ok, ENC_I16, ok, ENC_F32, 1, 2, 3, 14, 25, nullptr, ok, ok, msg, sizeof(msg)) == 1 && has("input_label or bad"), "input_label NULL");
    expect(enc_validate_maps(ok, ENC_U8, ok, ENC_I16, ok, ENC_F32, 1, 2, 3, 14, 25, ok, ok, nullptr, msg, sizeof(msg)) == 1 && has("input_label or bad"), "bad NULL");
    expect(enc_validate_maps(ok, ENC_I16, ok, ENC_I16, ok, ENC_F32, 1, 2, 3, 14, 25, ok, ok, ok, msg, sizeof(msg)) == 1 && has("label dtype 1"), "label int16");
    expect(enc_validate_maps(ok, ENC_U8, ok, ENC_U8, ok, ENC_F32, 1, 2, 3, 14, 25, ok, ok, ok, msg, sizeof(msg)) == 1 && has("inst dtype 0"), "inst uint8");
    expect(enc_validate_maps(ok, ENC_U8, ok, ENC_I16, ok, ENC_I16, 1, 2, 3, 14, 25, ok, ok, ok, msg, sizeof(msg)) == 1 && has("pose dtype 1"), "pose int16");
    expect(enc_validate_maps(ok, ENC_U8, ok, ENC_I16, ok, ENC_F32, 1, 2, 3, 0, 25, ok, ok, ok, msg, sizeof(msg)) == 1 && has("label_nc is 0"), "label_nc 0");
    expect(enc_validate_maps(ok, ENC_U8, ok, ENC_I16, ok, ENC_F32, 1, 2, 3, 257, 25, ok, ok, ok, msg, sizeof(msg)) == 1 && has("label_nc is 257"), "label_nc 257");
    expect(enc_validate_maps(ok, ENC_U8, ok, ENC_I16, ok, ENC_F32, 1, 2, 3, 14, -1, ok, ok, ok, msg, sizeof(msg)) == 1 && has("pose_ch is -1"), "pose_ch -1");
    expect(enc_validate_maps(ok, ENC_U8, ok, ENC_I16, ok, ENC_F32, 1, 2, 3, 14, 257, ok, ok, ok, msg, sizeof(msg)) == 1 && has("pose_ch is 257"), "pose_ch 257");
    expect(enc_validate_maps(ok, ENC_U8, ok, ENC_I16, nullptr, ENC_F32, 1, 2, 3, 14, 25, ok, ok, ok, msg, sizeof(msg)) == 1 && has("pose or pose_onehot is NULL"), "pose NULL");
    expect(enc_validate_maps(ok, ENC_U8, ok, ENC_I16, ok, ENC_F32, 1, 2, 3, 14, 25, ok, nullptr, ok, msg, sizeof(msg)) == 1 && has("pose or pose_onehot is NULL"), "pose_onehot NULL");
    expect(enc_validate_maps(ok, ENC_U8, ok, ENC_I16, odd, ENC_F32, 1, 2, 3, 14, 25, ok, ok, ok, msg, sizeof(msg)) == 1 && has("pose and pose_onehot must be aligned"), "pose misaligned");
    expect(enc_validate_maps(odd, ENC_F32, ok, ENC_I16, ok, ENC_F32, 1, 2, 3, 14, 25, ok, ok, ok, msg, sizeof(msg)) == 1 && has("label is not aligned"), "label misaligned");
    expect(enc_validate_maps(ok, ENC_U8, buf + 1, ENC_I16, ok, ENC_F32, 1, 2, 3, 14, 25, ok, ok, ok, msg, sizeof(msg)) == 1 && has("inst is not aligned"), "inst misaligned");
    expect(enc_validate_maps(ok, ENC_U8, ok, ENC_I16, ok, ENC_F32, 1, 2, 3, 14, 25, odd, ok, ok, msg, sizeof(msg)) == 1 && has("input_label and bad must be aligned"), "input_label misaligned");
    expect(enc_validate_maps(ok, ENC_U8, ok, ENC_I16, ok, ENC_F32, 0, 2, 3, 14, 25, ok, ok, ok, msg, sizeof(msg)) == 1 && has("bad sizes"), "N 0");
    expect(enc_validate_maps(ok, ENC_U8, ok, ENC_I16, ok, ENC_F32, 1, 2, -3, 14, 25, ok, ok, ok, msg, sizeof(msg)) == 1 && has("bad sizes"), "W negative");
    expect(enc_validate_maps(ok, ENC_U8, ok, ENC_I16, ok, ENC_F32, 4, 65536, 65536, 14, 25, ok, ok, ok, msg, sizeof(msg)) == 1 && has("below 2^31"), "H W overflows");
    expect(enc_validate_maps(ok, ENC_U8, ok, ENC_I16, ok, ENC_F32, 16, 4096, 4096, 14, 25, ok, ok, ok, msg, sizeof(msg)) == 1 && has("below 2^31"), "N C H W overflows");
    expect(enc_validate_maps(ok, ENC_U8, nullptr, 0, ok, ENC_F32, 16, 4096, 4096, 1, 8, ok, ok, ok, msg, sizeof(msg)) == 1 && has("below 2^31"), "the pose planes overflow");

    const size_t ws = IDX_WORKSPACE_BYTES;
    expect(IDX_BITMAP_AT == 0 && IDX_HEAD_AT == 262144 && IDX_PREFIX_AT == 262160 && ws == 524304 && IDX_PREFIX_AT % 16 == 0, "workspace layout");
    expect(idx_id_capacity(15) == 15 && idx_id_capacity(IDX_BITS) == IDX_BITS && idx_id_capacity(4L * 384 * 1248) == 4L * 384 * 1248 &&
               idx_id_capacity(3L * IDX_BITS) == IDX_BITS,
           "ids capacity");
    expect(idx_validate_build(ok, ENC_F32, 4, 384, 1248, ok, ws, ok, ok, 4L * 384 * 1248, msg, sizeof(msg)) == 0, "build at the full size");
    expect(idx_validate_build(ok, ENC_I16, 1, 3, 5, ok, ws, ok, nullptr, 15, msg, sizeof(msg)) == 0, "build without counts");
    expect(idx_validate_build(nullptr, ENC_F32, 1, 3, 5, ok, ws, ok, ok, 15, msg, sizeof(msg)) == 1 && has("inst is NULL"), "build inst NULL");
    expect(idx_validate_build(ok, ENC_U8, 1, 3, 5, ok, ws, ok, ok, 15, msg, sizeof(msg)) == 1 && has("inst dtype 0"), "build inst uint8");
    expect(idx_validate_build(odd, ENC_F32, 1, 3, 5, ok, ws, ok, ok, 15, msg, sizeof(msg)) == 1 && has("inst is not aligned"), "build inst misaligned");
    expect(idx_validate_build(ok, ENC_F32, 1, 3, 5, nullptr, ws, ok, ok, 15, msg, sizeof(msg)) == 1 && has("workspace is NULL"), "build workspace NULL");
    expect(idx_validate_build(ok, ENC_F32, 1, 3, 5, buf + 8, ws, ok, ok, 15, msg, sizeof(msg)) == 1 && has("workspace must be aligned"), "build workspace misaligned");
    expect(idx_validate_build(ok, ENC_F32, 1, 3, 5, ok, ws - 1, ok, ok, 15, msg, sizeof(msg)) == 1 && has("workspace holds"), "build workspace short");
    expect(idx_validate_build(ok, ENC_F32, 1, 3, 5, ok, ws, nullptr, ok, 15, msg, sizeof(msg)) == 1 && has("ids is NULL"), "build ids NULL");
    expect(idx_validate_build(ok, ENC_F32, 1, 3, 5, ok, ws, buf + 4, ok, 15, msg, sizeof(msg)) == 1 && has("aligned to 8"), "build ids misaligned");
    expect(idx_validate_build(ok, ENC_F32, 1, 3, 5, ok, ws, ok, buf + 4, 15, msg, sizeof(msg)) == 1 && has("aligned to 8"), "build counts misaligned");
    expect(idx_validate_build(ok, ENC_F32, 1, 3, 5, ok, ws, ok, ok, 14, msg, sizeof(msg)) == 1 && has("ids holds 14"), "build ids short");
    expect(idx_validate_build(ok, ENC_F32, 1, 0, 5, ok, ws, ok, ok, 15, msg, sizeof(msg)) == 1 && has("bad sizes"), "build H 0");
    expect(idx_validate_build(ok, ENC_F32, 2, 32768, 32768, ok, ws, ok, ok, IDX_BITS, msg, sizeof(msg)) == 1 && has("below 2^31"), "build overflows");
    expect(idx_validate_rank(ok, ENC_F32, 4, 384, 1248, ok, ws, ok, ok, msg, sizeof(msg)) == 0, "rank at the full size");
    expect(idx_validate_rank(ok, ENC_I32, 1, 3, 5, ok, ws, ok, nullptr, msg, sizeof(msg)) == 0, "rank without counts");
    expect(idx_validate_rank(ok, ENC_F32, 1, 3, 5, ok, ws, nullptr, ok, msg, sizeof(msg)) == 1 && has("seg is NULL"), "rank seg NULL");
    expect(idx_validate_rank(ok, ENC_F32, 1, 3, 5, ok, ws, odd, ok, msg, sizeof(msg)) == 1 && has("seg must be aligned"), "rank seg misaligned");
    expect(idx_validate_rank(ok, ENC_F32, 1, 3, 5, ok, ws, ok, buf + 4, msg, sizeof(msg)) == 1 && has("counts must be aligned"), "rank counts misaligned");
    expect(idx_validate_rank(ok, ENC_F32, 1, 3, 5, ok, 16, ok, ok, msg, sizeof(msg)) == 1 && has("workspace holds 16"), "rank workspace short");
    expect(idx_validate_rank(nullptr, ENC_F32, 1, 3, 5, ok, ws, ok, ok, msg, sizeof(msg)) == 1 && has("inst is NULL"), "rank inst NULL");
}

int main()
{
    walk_channels();
    walk_keys();
    const long first = IDX_KEY_MIN, last = IDX_KEY_MIN + IDX_BITS - 1;
    walk_scheme({31, 32, 33, 63, 64, 0, 64, 31});
    walk_scheme({first, last, last, 5, first, 5, 0, -1});
    walk_scheme({7});
    std::mt19937 rng(9);
    for (int round = 0; round < 6; round++) {
        std::vector<long> keys;
        const int n = 1 + (int)(rng() % 5000);
        const int spread = round < 3 ? 4000 : IDX_BITS;   // dense sets share words; sparse ones span the threads of the scan
        for (int i = 0; i < n; i++) keys.push_back(first + (long)(rng() % (unsigned)spread) * (round == 2 ? 1 : (IDX_BITS / spread)));
        walk_scheme(keys);
    }
    {   // every key of two whole steps of a wave of the scan, across the boundary to the wave before
        std::vector<long> keys;
        for (long b = 32L * IDX_WAVE_WORDS * 5 - 40; b < 32L * IDX_WAVE_WORDS * 5 + 32L * 256 * 2 + 40; b++) keys.push_back(first + b);
        walk_scheme(keys);
    }
    walk_validators();
    std::printf("encode_input_check: %ld pixels ranked, %d failures\n", ranked, failures);
    return failures ? 1 : 0;
}
