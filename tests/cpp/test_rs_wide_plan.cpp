// Host test of the wide Reed-Solomon coder's plan code (deoss_amd/csrc/rs_plan.hpp: gf_invert_n,
// rs_build_matrix_n, reconstruct_plan, rs_wide_table): no GPU, built plain and with ASan/UBSan by
// tests/test_rs_wide_plan.py.
//
//  1. rs_build_matrix_n equals rs_build_matrix for every geometry within 8 + 8; the top k rows of
//     every tested geometry are the identity; the parity row of 255 + 1 is all ones;
//  2. for seeded random erasure patterns of (10,4), (17,3), (64,32), (255,1) and (1,255): the inputs
//     are the first k present shards, the outputs every missing one, inverse x sub-matrix is the
//     identity, and the plan's rows applied to shards coded with a byte-wise loop give back the
//     originals; nothing missing gives no outputs; exactly m missing; all data missing where m >= k;
//  3. every entry of rs_wide_table (both nibble tables, all 8 byte lanes, the last group's unused
//     lanes zero) equals gf.mul, and low ^ high entry = the product of the whole byte;
//  4. a pattern with k - 1 present returns k - 1 (the "too few" status) whatever k is.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../deoss_amd/csrc/rs_plan.hpp"

using namespace dm_rsplan;

static int failures = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (failures++ < 20) {                                         \
                std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);  \
                std::fprintf(stderr, __VA_ARGS__);                         \
                std::fprintf(stderr, "\n");                                \
            }                                                              \
        }                                                                  \
    } while (0)

static std::vector<uint8_t> matrix(int k, int m) {
    std::vector<uint8_t> mat;
    CHECK(rs_build_matrix_n(k, m, mat) && mat.size() == (size_t)(k + m) * k, "rs_build_matrix_n(%d, %d)", k, m);
    for (int i = 0; i < k; i++)
        for (int j = 0; j < k; j++) CHECK(mat[(size_t)i * k + j] == (i == j), "(%d, %d) top row %d is no unit row", k, m, i);
    return mat;
}

static void check_matrices() {
    for (int k = 1; k <= kRsMaxIn; k++)
        for (int m = 1; m <= kRsMaxOut; m++) {
            std::vector<uint8_t> narrow;
            CHECK(rs_build_matrix(k, m, narrow), "rs_build_matrix(%d, %d)", k, m);
            CHECK(matrix(k, m) == narrow, "(%d, %d): the heap-backed matrix differs from the fixed-size one", k, m);
        }
    const std::vector<uint8_t> ones = matrix(255, 1);
    for (int j = 0; j < 255; j++) CHECK(ones[(size_t)255 * 255 + j] == 1, "255 + 1 parity row, column %d", j);
}

// shards (k + m) x n, coded byte by byte: shard k + i = sum_j mat[k + i][j] * shard j
static std::vector<uint8_t> coded(const std::vector<uint8_t>& mat, int k, int m, int n, std::mt19937& rng) {
    const Gf& g = gf();
    std::vector<uint8_t> sh((size_t)(k + m) * n);
    for (size_t i = 0; i < (size_t)k * n; i++) sh[i] = (uint8_t)rng();
    for (int i = k; i < k + m; i++)
        for (int b = 0; b < n; b++) {
            uint8_t acc = 0;
            for (int j = 0; j < k; j++) acc ^= g.mul(mat[(size_t)i * k + j], sh[(size_t)j * n + b]);
            sh[(size_t)i * n + b] = acc;
        }
    return sh;
}

static void check_pattern(const std::vector<uint8_t>& mat, int k, int m, const std::vector<uint8_t>& sh, int n,
                          const std::vector<uint8_t>& present, const char* what) {
    const Gf& g = gf();
    const int total = k + m;
    ReconstructPlan p;
    int np = 0;
    for (int i = 0; i < total; i++) np += present[i] != 0;
    const int got = reconstruct_plan(mat.data(), k, m, present.data(), p);
    if (np < k) {
        CHECK(got == np, "(%d, %d) %s: %d present gave %d", k, m, what, np, got);
        return;
    }
    CHECK(got == k, "(%d, %d) %s: status %d", k, m, what, got);
    if (got != k) return;
    // inputs: the first k present, in index order; outputs: every missing one
    std::vector<int> first, missing;
    for (int i = 0; i < total; i++) {
        if (!present[i]) missing.push_back(i);
        else if ((int)first.size() < k) first.push_back(i);
    }
    CHECK(p.inputs == first, "(%d, %d) %s: inputs", k, m, what);
    CHECK(p.outputs == missing, "(%d, %d) %s: outputs", k, m, what);
    if (missing.empty()) {
        CHECK(p.rows.empty(), "(%d, %d) %s: rows without outputs", k, m, what);
        return;
    }
    CHECK(p.rows.size() == missing.size() * (size_t)k, "(%d, %d) %s: %zu row bytes", k, m, what, p.rows.size());
    if (p.rows.size() != missing.size() * (size_t)k) return;
    // inverse x sub-matrix = identity
    std::vector<uint8_t> sub((size_t)k * k), inv, prod((size_t)k * k);
    for (int i = 0; i < k; i++) std::memcpy(&sub[(size_t)i * k], &mat[(size_t)first[i] * k], (size_t)k);
    CHECK(gf_invert_n(sub.data(), k, inv), "(%d, %d) %s: singular", k, m, what);
    gf_matmul_n(inv.data(), k, sub.data(), k, prod.data());
    for (int i = 0; i < k; i++)
        for (int j = 0; j < k; j++) CHECK(prod[(size_t)i * k + j] == (i == j), "(%d, %d) %s: inv x sub at %d,%d", k, m, what, i, j);
    // the rows give back the originals
    for (size_t t = 0; t < missing.size(); t++)
        for (int b = 0; b < n; b++) {
            uint8_t acc = 0;
            for (int j = 0; j < k; j++) acc ^= g.mul(p.rows[t * k + j], sh[(size_t)first[j] * n + b]);
            CHECK(acc == sh[(size_t)missing[t] * n + b], "(%d, %d) %s: shard %d byte %d", k, m, what, missing[t], b);
        }
}

static void check_plans() {
    const int shapes[][2] = {{10, 4}, {17, 3}, {64, 32}, {255, 1}, {1, 255}};
    std::mt19937 rng(20260);
    for (const auto& shp : shapes) {
        const int k = shp[0], m = shp[1], total = k + m, n = 7;
        const std::vector<uint8_t> mat = matrix(k, m);
        const std::vector<uint8_t> sh = coded(mat, k, m, n, rng);
        std::vector<uint8_t> present(total, 1);
        check_pattern(mat, k, m, sh, n, present, "nothing missing");
        auto lose = [&](int count, int lo, int hi) {   // `count` more shards of [lo, hi)
            for (int left = count; left > 0;) {
                const int i = lo + (int)(rng() % (uint32_t)(hi - lo));
                if (present[i]) {
                    present[i] = 0;
                    left--;
                }
            }
        };
        present.assign(total, 1);
        lose(1, 0, k);
        check_pattern(mat, k, m, sh, n, present, "one data shard missing");
        present.assign(total, 1);
        lose(1, k, total);
        check_pattern(mat, k, m, sh, n, present, "one parity shard missing");
        for (int rep = 0; rep < 3; rep++) {
            present.assign(total, 1);
            lose(m, 0, total);
            check_pattern(mat, k, m, sh, n, present, "exactly m missing");
            present.assign(total, 1);
            lose(1 + (int)(rng() % (uint32_t)m), 0, total);
            check_pattern(mat, k, m, sh, n, present, "random count missing");
        }
        if (m >= k) {
            present.assign(total, 1);
            for (int i = 0; i < k; i++) present[i] = 0;
            check_pattern(mat, k, m, sh, n, present, "all data missing");
        }
        // too few: k - 1 present (m + 1 missing), at the front, at the back and at random
        present.assign(total, 0);
        for (int i = 0; i < k - 1; i++) present[i] = 1;
        check_pattern(mat, k, m, sh, n, present, "k - 1 present, first");
        present.assign(total, 0);
        for (int i = 0; i < k - 1; i++) present[total - 1 - i] = 1;
        check_pattern(mat, k, m, sh, n, present, "k - 1 present, last");
        present.assign(total, 1);
        lose(m + 1, 0, total);
        check_pattern(mat, k, m, sh, n, present, "k - 1 present, random");
    }
}

static void check_tables() {
    const Gf& g = gf();
    const int shapes[][2] = {{10, 4}, {4, 12}, {9, 1}, {17, 3}, {16, 16}, {3, 255}, {255, 1}};
    for (const auto& shp : shapes) {
        const int k = shp[0], nout = shp[1];
        const int groups = (nout + kRsGroup - 1) / kRsGroup;
        std::vector<uint8_t> rows;
        if (k + nout <= kRsWideMaxShards) {
            const std::vector<uint8_t> mat = matrix(k, nout);
            rows.assign(mat.begin() + (size_t)k * k, mat.end());
        } else {   // any rows will do: every coefficient value in some lane
            rows.resize((size_t)nout * k);
            for (size_t i = 0; i < rows.size(); i++) rows[i] = (uint8_t)(i * 7 + 1);
        }
        const std::vector<uint64_t> tab = rs_wide_table(rows.data(), nout, k);
        CHECK(tab.size() == (size_t)groups * k * kRsWideEntries, "(%d, %d): %zu table entries", k, nout, tab.size());
        if (tab.size() != (size_t)groups * k * kRsWideEntries) continue;
        for (int gr = 0; gr < groups; gr++)
            for (int j = 0; j < k; j++) {
                const uint64_t* e = &tab[((size_t)gr * k + j) * kRsWideEntries];
                for (int i = 0; i < kRsGroup; i++) {
                    const int o = gr * kRsGroup + i;
                    const uint8_t c = o < nout ? rows[(size_t)o * k + j] : 0;
                    for (int x = 0; x < 16; x++) {
                        CHECK((uint8_t)(e[x] >> (8 * i)) == g.mul(c, (uint8_t)x), "(%d, %d) group %d input %d low %d lane %d", k,
                              nout, gr, j, x, i);
                        CHECK((uint8_t)(e[16 + x] >> (8 * i)) == g.mul(c, (uint8_t)(x << 4)),
                              "(%d, %d) group %d input %d high %d lane %d", k, nout, gr, j, x, i);
                    }
                    for (int x = 0; x < 256; x++)
                        CHECK((uint8_t)((e[x & 15] ^ e[16 + (x >> 4)]) >> (8 * i)) == g.mul(c, (uint8_t)x),
                              "(%d, %d) group %d input %d byte %d lane %d", k, nout, gr, j, x, i);
                }
            }
    }
}

int main() {
    check_matrices();
    check_plans();
    check_tables();
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("rs wide plan OK\n");
    return 0;
}
