// Host test of what a repair launch is built from (deoss_amd/csrc/rs_plan.hpp: repair_plan,
// RepairBatch, repair_add): no GPU, built plain and with ASan/UBSan by tests/test_repair_plan_host.py.
//
//  1. repair_plan over all 495 four-of-twelve patterns, every pattern of (3, 2) and (1, 8) and a
//     sample of (8, 8): the outputs are exactly the wanted fragments that are not present, in index
//     order, and every row is right: rows x (the inputs' rows of the coding matrix) is row j of the
//     coding matrix, which is what makes output j the original fragment j;
//  2. RepairBatch: plans are cached by (present, want), equal row sets share one table, the table of
//     a plan is rs_table of its rows;
//  3. the "some segment has more than k outputs" flag, which picks the kernel;
//  4. a batch mixing complete, narrow and wide segments: every descriptor's addresses;
//  5. too few fragments: nothing is added.
#include <cstdio>
#include <cstring>
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

static int bits(uint32_t x) {
    int n = 0;
    for (; x; x &= x - 1) n++;
    return n;
}

// rows[i] x (sub-matrix of the inputs) == mat[outputs[i]]
static bool rows_right(const uint8_t* mat, int k, const RepairPlan& p) {
    const Gf& g = gf();
    for (int i = 0; i < p.nout; i++)
        for (int c = 0; c < k; c++) {
            uint8_t acc = 0;
            for (int q = 0; q < k; q++) acc ^= g.mul(p.rows[i * k + q], mat[p.inputs[q] * k + c]);
            if (acc != mat[p.outputs[i] * k + c]) return false;
        }
    return true;
}

static void check_plans(int k, int m, uint32_t step) {
    std::vector<uint8_t> mat;
    CHECK(rs_build_matrix(k, m, mat), "rs_build_matrix(%d, %d)", k, m);
    const int total = k + m;
    size_t plans = 0;
    for (uint32_t pm = 0; pm < (1u << total); pm += step) {
        uint8_t present[kRsMaxIn + kRsMaxOut], want[kRsMaxIn + kRsMaxOut];
        for (int j = 0; j < total; j++) present[j] = pm >> j & 1;
        // want: everything (null), and a pattern-dependent subset that includes present fragments
        for (int pass = 0; pass < 2; pass++) {
            const uint32_t wm = pass ? (pm * 2654435761u >> 7) & ((1u << total) - 1) : (1u << total) - 1;
            for (int j = 0; j < total; j++) want[j] = wm >> j & 1;
            RepairPlan p;
            const int got = repair_plan(mat.data(), k, m, present, pass ? want : nullptr, p);
            if (bits(pm) < k) {
                CHECK(got == bits(pm), "(%d, %d) pattern %x: too few reported as %d", k, m, pm, got);
                continue;
            }
            CHECK(got == k, "(%d, %d) pattern %x: %d", k, m, pm, got);
            int n = 0, nin = 0;
            for (int j = 0; j < total; j++) {
                if (present[j] && nin < k) CHECK(p.inputs[nin++] == j, "(%d, %d) pattern %x: input %d", k, m, pm, j);
                if (!present[j] && (wm >> j & 1)) {
                    CHECK(n < p.nout && p.outputs[n] == j, "(%d, %d) pattern %x want %x: output %d", k, m, pm, wm, j);
                    n++;
                }
            }
            CHECK(n == p.nout && p.nout <= m, "(%d, %d) pattern %x want %x: %d outputs, expected %d", k, m, pm, wm, p.nout, n);
            CHECK(rows_right(mat.data(), k, p), "(%d, %d) pattern %x want %x: rows", k, m, pm, wm);
            plans++;
        }
    }
    std::printf("plans %d %d %zu\n", k, m, plans);
}

static uint8_t* addr(uint64_t x) { return reinterpret_cast<uint8_t*>(x); }   // never dereferenced

static void check_batch() {
    const int k = 4, m = 8, total = 12;
    std::vector<uint8_t> mat;
    CHECK(rs_build_matrix(k, m, mat), "rs_build_matrix");
    RepairBatch b{mat.data(), k, m};
    const uint64_t frag = 4096;
    struct Case {
        uint32_t present, wanted;
        int nout;
    };
    // complete; narrow (2 out); wide (8 out); narrow again with the same pattern (cached); a present
    // fragment that is not among the first k and a subset wanted; absent and not wanted (NULL)
    const Case cases[] = {{0xfff, 0, 0},     {0xff3, 0x00c, 2}, {0x0f0, 0xf0f, 8}, {0xff3, 0x00c, 2},
                          {0x3f0, 0x00f, 4}, {0x0f1, 0xe00, 3}, {0x0f0, 0xf0f, 8}};
    const size_t ncase = sizeof(cases) / sizeof(cases[0]);
    for (size_t s = 0; s < ncase; s++) {
        uint8_t* ptr[12];
        uint8_t present[12];
        for (int j = 0; j < total; j++) {
            present[j] = cases[s].present >> j & 1;
            const bool given = present[j] || (cases[s].wanted >> j & 1);
            ptr[j] = given ? addr(0x100000 + (s * total + j) * frag) : nullptr;
        }
        CHECK(!b.any_wide || s > 2, "any_wide before the first wide segment");
        CHECK(repair_add(b, ptr, present) == k, "repair_add of case %zu", s);
        CHECK(b.any_wide == (s >= 2), "any_wide after case %zu", s);
        CHECK(b.any_out == (s >= 1), "any_out after case %zu", s);
    }
    CHECK(b.desc.size() == ncase, "%zu descriptors", b.desc.size());
    CHECK(b.plans.size() == 5, "%zu cached plans for 5 distinct (present, want)", b.plans.size());
    const size_t ntab = b.tabs.size() / ((size_t)k * 256);
    CHECK(ntab == 4 && b.tab_of.size() == 4, "%zu tables for 4 distinct non-empty row sets", ntab);
    CHECK(b.desc[1].table == b.desc[3].table && b.desc[2].table == b.desc[6].table, "equal patterns share a table");
    CHECK(b.desc[1].table != b.desc[2].table && b.desc[4].table != b.desc[5].table, "different rows, different tables");
    for (size_t s = 0; s < ncase; s++) {
        const dm::RsRestoreDesc& ds = b.desc[s];
        CHECK((int)ds.nout == cases[s].nout, "case %zu: nout %u", s, ds.nout);
        int nin = 0, n = 0;
        for (int j = 0; j < total; j++) {
            uint8_t* at = addr(0x100000 + (s * total + j) * frag);
            if ((cases[s].present >> j & 1) && nin < k) {
                CHECK(ds.in[nin] == at, "case %zu: input %d address", s, nin);
                nin++;
            }
            if (!(cases[s].present >> j & 1) && (cases[s].wanted >> j & 1)) {
                CHECK(ds.out[n] == at, "case %zu: output %d address", s, n);
                n++;
            }
        }
        CHECK(n == (int)ds.nout, "case %zu: %d outputs", s, n);
        for (int i = n; i < kRsMaxOut; i++) CHECK(ds.out[i] == nullptr, "case %zu: output slot %d not empty", s, i);
        if (ds.nout) {   // the table is rs_table of the plan's rows
            uint8_t present[12], want[12];
            for (int j = 0; j < total; j++) {
                present[j] = cases[s].present >> j & 1;
                want[j] = cases[s].wanted >> j & 1;
            }
            RepairPlan p;
            CHECK(repair_plan(mat.data(), k, m, present, want, p) == k, "case %zu: plan", s);
            const std::vector<uint64_t> t = rs_table(p.rows, p.nout, k);
            CHECK(std::memcmp(t.data(), b.tabs.data() + (size_t)ds.table * k * 256, t.size() * 8) == 0, "case %zu: table", s);
        }
    }
    // a narrow-only batch keeps the flag down; exactly k outputs is still narrow
    RepairBatch nb{mat.data(), k, m};
    uint8_t* ptr[12];
    uint8_t present[12];
    for (int j = 0; j < total; j++) {
        present[j] = j >= 8;
        ptr[j] = (j < 4 || j >= 8) ? addr(0x200000 + j * frag) : nullptr;
    }
    CHECK(repair_add(nb, ptr, present) == k && nb.desc[0].nout == 4 && nb.any_out && !nb.any_wide, "k outputs are narrow");
    ptr[4] = addr(0x200000 + 4 * frag);
    CHECK(repair_add(nb, ptr, present) == k && nb.desc[1].nout == 5 && nb.any_wide, "k + 1 outputs are wide");
    // too few: nothing is added; a present flag without an address does not count
    for (int j = 0; j < total; j++) present[j] = j < 3;
    CHECK(repair_add(nb, ptr, present) == 3 && nb.desc.size() == 2, "3 of 12 is too few");
    for (int j = 0; j < total; j++) present[j] = 1;
    for (int j = 0; j < total; j++) ptr[j] = j < 2 ? addr(0x300000 + j * frag) : nullptr;
    CHECK(repair_add(nb, ptr, present) == 2 && nb.desc.size() == 2, "present without an address");
}

int main() {
    check_plans(4, 8, 1);
    check_plans(3, 2, 1);
    check_plans(1, 8, 1);
    check_plans(8, 8, 37);
    check_batch();
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("repair plan OK\n");
    return 0;
}
