// Host test of what the Reed-Solomon entry points decide before a launch (deoss_amd/csrc/rs_plan.hpp)
// and of the restore path's file helpers (deoss_amd/csrc/fp_files.hpp: read_files, pwrite_all): no
// GPU, built plain and with ASan/UBSan by tests/test_rs_plan_host.py.  argv[1]: an empty scratch
// directory.
//
//  1. the (4, 8) and (8, 8) coding matrices are printed ("matrix k m row row ..."; the wrapper
//     compares them with tests/golden/rs_golden.json); their top k rows are the identity;
//  2. rs_pick_inputs over all 495 four-of-twelve patterns and every pattern of (3, 2) and (1, 8):
//     the inputs are the first k present in index order, inverse x sub-matrix is the identity,
//     fewer than k present is "too few" with the right counts;
//  3. restore_plan: the outputs are exactly the data fragments missing or not in place, a present
//     data fragment gets a unit row, everything in place gives nout == 0;
//  4. rt_select: exactly k good, more than k, fewer than k, entries already marked bad;
//  5. RestoreBatch: all 495 patterns in one batch (descriptors, table sharing, addresses), a segment
//     in place, a segment with too few;
//  6. read_files with more and fewer readers than files, a missing and a short file; pwrite_all at
//     a non-zero offset.
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../deoss_amd/csrc/fp_files.hpp"
#include "../../deoss_amd/csrc/rs_plan.hpp"

using namespace dm_rsplan;
using namespace dm_fp;

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
    CHECK(rs_build_matrix(k, m, mat) && mat.size() == (size_t)(k + m) * k, "rs_build_matrix(%d, %d)", k, m);
    return mat;
}

static void check_matrices() {
    const int shapes[][2] = {{4, 8}, {8, 8}};
    for (const auto& sh : shapes) {
        const int k = sh[0], m = sh[1];
        const std::vector<uint8_t> mat = matrix(k, m);
        std::printf("matrix %d %d", k, m);
        for (int i = 0; i < k + m; i++) {
            std::printf(" ");
            for (int j = 0; j < k; j++) std::printf("%02x", mat[(size_t)i * k + j]);
        }
        std::printf("\n");
        for (int i = 0; i < k; i++)
            for (int j = 0; j < k; j++) CHECK(mat[(size_t)i * k + j] == (i == j), "(%d, %d) top row %d is no unit row", k, m, i);
    }
}

// sub-matrix of the inputs x inv == identity
static bool inverts(const uint8_t* mat, int k, const int* inputs, const uint8_t* inv) {
    const Gf& g = gf();
    for (int a = 0; a < k; a++)
        for (int b = 0; b < k; b++) {
            uint8_t acc = 0;
            for (int q = 0; q < k; q++) acc ^= g.mul(inv[a * k + q], mat[inputs[q] * k + b]);
            if (acc != (uint8_t)(a == b)) return false;
        }
    return true;
}

static int bits(uint32_t x) {
    int n = 0;
    for (; x; x &= x - 1) n++;
    return n;
}

// every pattern of (k, m) with at least `lo` and at most `hi` fragments present
static std::vector<uint32_t> patterns(int total, int lo, int hi) {
    std::vector<uint32_t> out;
    for (uint32_t p = 0; p < (1u << total); p++)
        if (bits(p) >= lo && bits(p) <= hi) out.push_back(p);
    return out;
}

static void check_pick(int k, int m, int lo, int hi, size_t want_patterns) {
    const int total = k + m;
    const std::vector<uint8_t> mat = matrix(k, m);
    const std::vector<uint32_t> pats = patterns(total, lo, hi);
    CHECK(pats.size() == want_patterns, "(%d, %d): %zu patterns", k, m, pats.size());
    for (uint32_t p : pats) {
        uint8_t present[kRsMaxIn + kRsMaxOut];
        std::vector<int> first;
        for (int i = 0; i < total; i++) {
            present[i] = (p >> i) & 1;
            if (present[i] && (int)first.size() < k) first.push_back(i);
        }
        int inputs[kRsMaxIn];
        uint8_t inv[kRsMaxIn * kRsMaxIn];
        const int got = rs_pick_inputs(mat.data(), k, m, present, inputs, inv);
        CHECK(got == (bits(p) < k ? bits(p) : k), "(%d, %d) pattern %x: %d of %d present reported as %d", k, m, p, bits(p), k,
              got);
        if (got != k) continue;
        CHECK(std::vector<int>(inputs, inputs + k) == first, "(%d, %d) pattern %x: inputs", k, m, p);
        CHECK(inverts(mat.data(), k, inputs, inv), "(%d, %d) pattern %x: inverse", k, m, p);
    }
}

static void check_restore_plan() {
    const int k = 4, m = 8, total = 12;
    const std::vector<uint8_t> mat = matrix(k, m);
    for (uint32_t p : patterns(total, k, total))
        for (uint32_t place = 0; place < 16; place++) {   // in_place may also name absent fragments: ignored
            uint8_t present[12], in_place[4];
            for (int i = 0; i < total; i++) present[i] = (p >> i) & 1;
            for (int j = 0; j < k; j++) in_place[j] = (place >> j) & 1;
            RestorePlan rp;
            CHECK(restore_plan(mat.data(), k, m, present, in_place, rp) == k, "pattern %x", p);
            std::vector<int> want;
            for (int j = 0; j < k; j++)
                if (!(present[j] && in_place[j])) want.push_back(j);
            CHECK(std::vector<int>(rp.outputs, rp.outputs + rp.nout) == want, "pattern %x place %x: outputs", p, place);
            if ((p & 15) == 15 && place == 15) CHECK(rp.nout == 0, "everything in place: nout %d", rp.nout);
            for (int o = 0; o < rp.nout; o++) {
                const int j = rp.outputs[o];
                if (!present[j]) continue;
                int at = -1;   // a present data fragment is an input: its row is the unit row of that input
                for (int q = 0; q < k; q++)
                    if (rp.inputs[q] == j) at = q;
                CHECK(at >= 0, "pattern %x: present data fragment %d is no input", p, j);
                for (int q = 0; q < k; q++)
                    CHECK(rp.rows[o * k + q] == (uint8_t)(q == at), "pattern %x output %d: no unit row", p, j);
            }
            if (place == 0) {   // a null in_place means nothing is in place
                RestorePlan rn;
                CHECK(restore_plan(mat.data(), k, m, present, nullptr, rn) == k && rn.nout == k &&
                          std::memcmp(rn.rows, rp.rows, (size_t)k * k) == 0, "pattern %x: null in_place", p);
            }
        }
    uint8_t few[12] = {0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    RestorePlan rp;
    CHECK(restore_plan(mat.data(), k, m, few, nullptr, rp) == 3, "3 of 12 must report 3 present");
    // a matrix with two equal rows among the inputs has no inverse
    std::vector<uint8_t> twice = mat;
    std::memcpy(twice.data() + 6 * k, twice.data() + 1 * k, (size_t)k);
    CHECK(restore_plan(twice.data(), k, m, few, nullptr, rp) == 3, "too few comes before singular");
    few[3] = 1;
    CHECK(restore_plan(twice.data(), k, m, few, nullptr, rp) == kPlanSingular, "equal rows 1 and 6 must be singular");
}

static void check_select() {
    const int k = 4, total = 12;
    //                     exactly k            more than k                fewer than k           a bad one beside k good
    const uint8_t is_good[4 * 12] = {0, 1, 0, 1, 0, 0, 1, 0, 0, 0, 0, 1,  1, 0, 1, 1, 0, 1, 0, 1, 1, 0, 0, 0,
                                     0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0,  1, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0};
    const uint8_t* good[4 * 12];   // a good fragment has an address
    for (int i = 0; i < 4 * 12; i++) good[i] = is_good[i] ? is_good + i : nullptr;
    std::vector<uint8_t> fst(4 * 12, kFragAbsent), sst(4, kSegOk);
    fst[2 * 12 + 3] = kFragBad;
    fst[3 * 12 + 1] = kFragBad;
    CHECK(!rt_select(k, total, 4, good, fst.data(), sst.data()), "a segment with too few must return false");
    const uint8_t U = kFragUsed, S = kFragSpare, B = kFragBad;
    const uint8_t want[4 * 12] = {0, U, 0, U, 0, 0, U, 0, 0, 0, 0, U,  U, 0, U, U, 0, U, 0, S, S, 0, 0, 0,
                                  0, 0, S, B, 0, 0, 0, S, 0, S, 0, 0,  U, B, U, 0, U, 0, 0, 0, 0, U, 0, 0};
    CHECK(std::memcmp(fst.data(), want, sizeof want) == 0, "fragment statuses");
    CHECK(sst == std::vector<uint8_t>({kSegOk, kSegOk, kSegTooFew, kSegOk}), "segment statuses");
    std::vector<uint8_t> f2(2 * 12, 0), s2(2, 0);
    CHECK(rt_select(k, total, 2, good, f2.data(), s2.data()) && s2 == std::vector<uint8_t>(2, kSegOk), "two good segments");
}

static void check_batch() {
    const int k = 4, m = 8, total = 12;
    const uint64_t frag = 64, seg = k * frag;
    const std::vector<uint8_t> mat = matrix(k, m);
    const std::vector<uint32_t> pats = patterns(total, k, k);
    CHECK(pats.size() == 495, "%zu patterns", pats.size());
    // addresses only: the object, and a pool that holds every fragment somewhere else
    std::vector<uint8_t> obj(pats.size() * seg), pool(pats.size() * total * frag);
    RestoreBatch b{mat.data(), k, m};
    std::set<std::string> row_sets;
    std::set<uint32_t> keys;
    for (size_t t = 0; t < pats.size(); t++) {
        const uint8_t* frags[12];
        uint8_t present[12], in_place[4] = {0, 0, 0, 0};
        uint32_t key = pats[t];
        for (int j = 0; j < total; j++) {
            present[j] = (pats[t] >> j) & 1;
            frags[j] = present[j] ? pool.data() + (t * total + j) * frag : nullptr;
            if (j < k && present[j] && (t + j) % 3 == 0) {   // some data fragments lie in place
                frags[j] = obj.data() + t * seg + j * frag;
                in_place[j] = 1;
                key |= 1u << (16 + j);
            }
        }
        keys.insert(key);
        CHECK(restore_add(b, frags, obj.data() + t * seg, frag) == k, "segment %zu", t);
        CHECK(b.desc.size() == t + 1, "one descriptor per segment");
        RestorePlan rp;
        CHECK(restore_plan(mat.data(), k, m, present, in_place, rp) == k, "plan %zu", t);
        const dm::RsRestoreDesc& ds = b.desc[t];
        CHECK((int)ds.nout == rp.nout, "segment %zu: nout %u, plan %d", t, ds.nout, rp.nout);
        for (int q = 0; q < k; q++) CHECK(ds.in[q] == frags[rp.inputs[q]], "segment %zu: input %d", t, q);
        for (int o = 0; o < rp.nout; o++)
            CHECK(ds.out[o] == obj.data() + t * seg + (uint64_t)rp.outputs[o] * frag, "segment %zu: output %d", t, o);
        if (rp.nout) {
            row_sets.insert(std::string(reinterpret_cast<const char*>(rp.rows), (size_t)rp.nout * k));
            const std::vector<uint64_t> tab = rs_table(rp.rows, rp.nout, k);
            CHECK(((size_t)ds.table + 1) * k * 256 <= b.tabs.size() &&
                      std::memcmp(b.tabs.data() + (size_t)ds.table * k * 256, tab.data(), tab.size() * 8) == 0,
                  "segment %zu: table %u is not its rows' table", t, ds.table);
        }
    }
    CHECK(b.any_out, "any_out");
    CHECK(b.tabs.size() == row_sets.size() * (size_t)k * 256, "%zu tables for %zu row sets", b.tabs.size() / (k * 256),
          row_sets.size());
    CHECK(row_sets.size() <= keys.size() && b.plans.size() == keys.size(), "%zu row sets, %zu keys, %zu plans",
          row_sets.size(), keys.size(), b.plans.size());

    // every data fragment in place: nout == 0, and alone it leaves any_out false
    RestoreBatch one{mat.data(), k, m};
    const uint8_t* frags[12] = {};
    for (int j = 0; j < k; j++) frags[j] = obj.data() + j * frag;
    frags[7] = pool.data();
    CHECK(restore_add(one, frags, obj.data(), frag) == k && one.desc.size() == 1 && one.desc[0].nout == 0 && !one.any_out &&
              one.tabs.empty(), "a segment in place");
    // too few: reported, nothing added
    frags[2] = nullptr;
    frags[7] = nullptr;
    CHECK(restore_add(one, frags, obj.data(), frag) == 3 && one.desc.size() == 1, "too few: 3 present, nothing added");
}

static void check_files(const std::string& root) {
    const size_t n = 5;
    const uint64_t len = 70001;
    std::vector<std::string> paths;
    std::vector<uint8_t> all(n * len);
    for (size_t i = 0; i < all.size(); i++) all[i] = (uint8_t)(i * 131 + (i >> 9));
    for (size_t i = 0; i < n; i++) {
        paths.push_back(root + "/frag" + std::to_string(i));
        CHECK(write_whole(paths[i], all.data() + i * len, len).empty(), "write %zu", i);
    }
    for (size_t readers : {(size_t)8, (size_t)2, (size_t)1}) {
        std::vector<uint8_t> buf(n * len + 1, 0xEE);
        const std::string e = read_files(paths.data(), n, len, buf.data(), readers);
        CHECK(e.empty(), "read_files with %zu readers: %s", readers, e.c_str());
        CHECK(std::memcmp(buf.data(), all.data(), all.size()) == 0 && buf[n * len] == 0xEE, "content with %zu readers", readers);
    }
    std::vector<uint8_t> buf(n * len);
    CHECK(read_files(paths.data(), 0, len, buf.data(), 8).empty(), "no files");
    std::vector<std::string> bad = paths;
    bad[3] = root + "/missing";
    std::string e = read_files(bad.data(), n, len, buf.data(), 2);
    CHECK(e == "open " + bad[3] + ": no such file or directory", "missing file: '%s'", e.c_str());
    bad[3] = root + "/short";
    CHECK(write_whole(bad[3], all.data(), len - 1).empty(), "write short");
    e = read_files(bad.data(), n, len, buf.data(), 8);
    CHECK(e == "read " + bad[3] + ": unexpected EOF", "short file: '%s'", e.c_str());
    bad[3] = root;   // a directory opens, and cannot be read
    e = read_files(bad.data(), n, len, buf.data(), 3);
    CHECK(e == "read " + root + ": " + go_errno(EISDIR), "directory: '%s'", e.c_str());

    // pwrite_all at a non-zero offset, out of order
    const std::string outp = root + "/out";
    FdGuard fd;
    fd.fd = ::open(outp.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    CHECK(fd.fd >= 0, "open %s", outp.c_str());
    CHECK(pwrite_all(fd.fd, outp, all.data() + len, 2 * len, len).empty(), "pwrite_all at an offset");
    CHECK(pwrite_all(fd.fd, outp, all.data(), len, 0).empty() && pwrite_all(fd.fd, outp, all.data(), 0, 5).empty(),
          "pwrite_all at 0");
    std::vector<uint8_t> got(3 * len);
    std::vector<std::string> op(1, outp);
    CHECK(read_files(op.data(), 1, 3 * len, got.data(), 1).empty() && std::memcmp(got.data(), all.data(), 3 * len) == 0,
          "pwrite_all content");
    FdGuard ro;
    ro.fd = ::open(outp.c_str(), O_RDONLY | O_CLOEXEC);
    e = pwrite_all(ro.fd, outp, all.data(), 10, 0);
    CHECK(e == "write " + outp + ": " + go_errno(EBADF), "pwrite_all error: '%s'", e.c_str());
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <empty scratch directory>\n", argv[0]);
        return 2;
    }
    check_matrices();
    check_pick(4, 8, 4, 4, 495);
    check_pick(4, 8, 0, 3, 1 + 12 + 66 + 220);
    check_pick(3, 2, 0, 5, 32);
    check_pick(1, 8, 0, 9, 512);
    check_restore_plan();
    check_select();
    check_batch();
    check_files(argv[1]);
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("rs plan OK\n");
    return 0;
}
