// Host test of the striped cipher file path's plan: the stripes of a window (fp_layout.hpp:
// fp_stripe_pitch, fp_stripe_plan) and the plaintext each one brings (cipher_scheme.hpp:
// stripe_span), as fp_striped_pass combines them.  Stand-alone, no GPU; built plain and with
// ASan/UBSan by tests/test_cipher_stripes_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../deoss_amd/csrc/cipher_scheme.hpp"
#include "../../deoss_amd/csrc/fp_layout.hpp"

static int g_fail = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            if (++g_fail > 20) std::exit(1);                                \
        }                                                                   \
    } while (0)

static uint64_t check_plan(int k, int m, uint64_t segment, uint64_t slot_cap, uint64_t ns) {
    const dm_fp::FpLayout L(k, m, segment);
    const uint64_t P = segment - dm_cipher::kBlock;
    const uint64_t W = dm_fp::fp_stripe_pitch(slot_cap, ns);
    EXPECT(W >= 64 && W % 64 == 0 && (W == 64 || W * ns <= slot_cap));
    std::vector<uint64_t> so, sw;
    dm_fp::fp_stripe_plan(L, W, so, sw);
    EXPECT(!so.empty() && so.size() == sw.size());
    uint64_t at = 0, plain_at = 0, pads = 0;
    for (size_t j = 0; j < so.size(); j++) {
        const uint64_t o = so[j], w = sw[j];
        // the stripes tile the segment in order, in whole SHA-256 blocks, inside a slot row
        EXPECT(o == at && w >= 64 && w % 64 == 0 && w <= W && o + w <= segment);
        // no stripe crosses a fragment boundary
        EXPECT(o / L.frag == (o + w - 1) / L.frag);
        const dm_cipher::StripeSpan s = dm_cipher::stripe_span(o, w, segment);
        // the plaintext spans tile [0, P) exactly once and in order, in whole AES blocks
        EXPECT(s.off == plain_at && s.off == o && s.len > 0 && s.len % 16 == 0 && s.off + s.len <= P);
        EXPECT(s.blk_lo() * 16 == s.off && s.blk_hi() * 16 == s.off + s.len && s.blk_lo() < s.blk_hi());
        // exactly the last stripe carries the padding block, and 16 bytes less of plaintext
        const bool last = j + 1 == so.size();
        EXPECT(s.pad == last);
        EXPECT(s.len == (last ? w - 16 : w));
        pads += s.pad ? 1 : 0;
        at = o + w;
        plain_at = s.off + s.len;
    }
    EXPECT(at == segment && plain_at == P && pads == 1);
    return so.size();
}

int main() {
    const uint64_t segments[] = {256, 4096, 32ull << 20};
    uint64_t plans = 0, stripes = 0;
    for (const uint64_t segment : segments)
        for (const uint64_t ns : {4ull, 5ull, 11ull, 16ull, 257ull})
            for (const uint64_t slot : {1ull, 8192ull, 12345ull, 1ull << 20, 64ull << 20, 1ull << 30}) {
                if (segment > (1u << 20) && slot / ns < 4096) continue;   // millions of 64-byte stripes: minutes under ASan
                stripes += check_plan(4, 8, segment, slot, ns);
                plans++;
            }
    // other codes: 2 + 1 and 10 + 4 (fragment = segment / k, whole 64-byte blocks)
    stripes += check_plan(2, 1, 4096, 8192, 7);
    stripes += check_plan(10, 4, 640 * 10, 4096, 9);
    // the spans of a hand-made plan
    {
        const dm_cipher::StripeSpan a = dm_cipher::stripe_span(0, 64, 256), b = dm_cipher::stripe_span(192, 64, 256);
        EXPECT(a.off == 0 && a.len == 64 && !a.pad && a.blk_lo() == 0 && a.blk_hi() == 4);
        EXPECT(b.off == 192 && b.len == 48 && b.pad && b.blk_lo() == 12 && b.blk_hi() == 15);
        const dm_cipher::StripeSpan c = dm_cipher::stripe_span(0, 256, 256);   // one stripe: the whole piece
        EXPECT(c.off == 0 && c.len == 240 && c.pad);
    }
    if (g_fail) return 1;
    std::printf("cipher stripes OK (%llu plans, %llu stripes)\n", (unsigned long long)(plans + 2), (unsigned long long)stripes);
    return 0;
}
