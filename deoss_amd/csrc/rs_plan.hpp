// rs_plan.hpp -- what the Reed-Solomon entry points decide before a launch (pure host code, no
// HIP): the GF(2^8) arithmetic behind the coding tables, a reconstruction's inputs and rows, a
// restore's statuses, and the descriptors and tables of one restore or one repair launch.
//
// Shared by rs_capi.inl, restore_capi.inl, repair_capi.inl, rs_kernels.hpp (the shard limits and the
// descriptor its kernels read) and the host tests (tests/cpp/test_rs_plan.cpp,
// tests/cpp/test_repair_plan.cpp and tests/cpp/test_rs_wide_plan.cpp, plain and ASan/UBSan, no GPU).
// Mirrors klauspost/reedsolomon v1.12.4: its default matrix, and Reconstruct's choice of inputs.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace dm {

constexpr int kRsMaxIn = 8;
constexpr int kRsMaxOut = 8;

// One restored segment: the fragments to read, the data fragments to write -- those not yet at their
// final address in the object -- and the coding table that maps one to the other (a missing
// fragment's row comes from the inverse sub-matrix, a present one elsewhere has a unit row).  A
// repaired segment uses the same descriptor: out holds its missing fragments, data or parity.
struct RsRestoreDesc {
    const uint8_t* in[kRsMaxIn];   // the first k usable fragments, in index order
    uint8_t* out[kRsMaxIn];        // addresses of the fragments to write (restore: nout <= k; repair: <= kRsMaxOut)
    uint32_t nout;                 // 0: every data fragment is in place, nothing to do
    uint32_t table;                // index into RsRestoreArgs::tables
};

}  // namespace dm

namespace dm_rsplan {

using dm::kRsMaxIn;
using dm::kRsMaxOut;

struct Gf {
    uint8_t exp[510];
    uint8_t log[256];
    Gf() {
        unsigned x = 1;
        for (int i = 0; i < 255; i++) {
            exp[i] = (uint8_t)x;
            log[x] = (uint8_t)i;
            x <<= 1;
            if (x & 0x100) x ^= 0x11d;   // x^8 + x^4 + x^3 + x^2 + 1 (klauspost "29")
        }
        for (int i = 255; i < 510; i++) exp[i] = exp[i - 255];
        log[0] = 0;
    }
    uint8_t mul(uint8_t a, uint8_t b) const { return (a && b) ? exp[log[a] + log[b]] : 0; }
    uint8_t inv(uint8_t a) const { return exp[255 - log[a]]; }
    uint8_t pow(uint8_t a, int n) const { return n == 0 ? 1 : (a == 0 ? 0 : exp[(log[a] * n) % 255]); }
};

inline const Gf& gf() {
    static const Gf g;
    return g;
}

// Gauss-Jordan inverse of a k x k GF(2^8) matrix; false if singular.
inline bool gf_invert(const uint8_t* m, int k, uint8_t* out) {
    const Gf& g = gf();
    uint8_t w[kRsMaxIn][2 * kRsMaxIn];
    for (int r = 0; r < k; r++)
        for (int c = 0; c < k; c++) {
            w[r][c] = m[r * k + c];
            w[r][k + c] = (uint8_t)(r == c);
        }
    for (int c = 0; c < k; c++) {
        int p = c;
        while (p < k && w[p][c] == 0) p++;
        if (p == k) return false;
        if (p != c)
            for (int j = 0; j < 2 * k; j++) std::swap(w[p][j], w[c][j]);
        const uint8_t s = g.inv(w[c][c]);
        for (int j = 0; j < 2 * k; j++) w[c][j] = g.mul(w[c][j], s);
        for (int r = 0; r < k; r++) {
            if (r == c || w[r][c] == 0) continue;
            const uint8_t f = w[r][c];
            for (int j = 0; j < 2 * k; j++) w[r][j] ^= g.mul(f, w[c][j]);
        }
    }
    for (int r = 0; r < k; r++)
        for (int c = 0; c < k; c++) out[r * k + c] = w[r][k + c];
    return true;
}

// klauspost buildMatrix: vandermonde(total, k) x inverse(top k x k), (k + m) x k row-major.
inline bool rs_build_matrix(int k, int m, std::vector<uint8_t>& mat) {
    const Gf& g = gf();
    const int total = k + m;
    std::vector<uint8_t> vm((size_t)total * k);
    for (int i = 0; i < total; i++)
        for (int j = 0; j < k; j++) vm[(size_t)i * k + j] = g.pow((uint8_t)i, j);
    uint8_t inv[kRsMaxIn * kRsMaxIn];
    if (!gf_invert(vm.data(), k, inv)) return false;
    mat.assign((size_t)total * k, 0);
    for (int i = 0; i < total; i++)
        for (int j = 0; j < k; j++) {
            uint8_t acc = 0;
            for (int t = 0; t < k; t++) acc ^= g.mul(vm[(size_t)i * k + t], inv[t * k + j]);
            mat[(size_t)i * k + j] = acc;
        }
    return true;
}

// Lookup table of `rows` (nout x k, row-major): entry [j][x] byte i = rows[i][j] * x.
inline std::vector<uint64_t> rs_table(const uint8_t* rows, int nout, int k) {
    const Gf& g = gf();
    std::vector<uint64_t> t((size_t)k * 256, 0);
    for (int j = 0; j < k; j++)
        for (int x = 0; x < 256; x++) {
            uint64_t e = 0;
            for (int i = 0; i < nout; i++) e |= (uint64_t)g.mul(rows[i * k + j], (uint8_t)x) << (8 * i);
            t[(size_t)j * 256 + x] = e;
        }
    return t;
}

constexpr int kPlanSingular = -1;

// The inputs of one pattern (klauspost's Reconstruct): the first k present fragments in index order,
// and the inverse of their rows of the coding matrix `mat` ((k + m) x k).  Returns k; or, without a
// plan, how many fragments (< k: too few) are present, or kPlanSingular.
inline int rs_pick_inputs(const uint8_t* mat, int k, int m, const uint8_t* present, int* inputs, uint8_t* inv) {
    int nv = 0;
    for (int i = 0; i < k + m && nv < k; i++)
        if (present[i]) inputs[nv++] = i;
    if (nv < k) return nv;
    uint8_t sub[kRsMaxIn * kRsMaxIn] = {};
    for (int i = 0; i < k; i++) std::memcpy(sub + i * k, mat + inputs[i] * k, (size_t)k);
    return gf_invert(sub, k, inv) ? k : kPlanSingular;
}

static_assert(kRsMaxOut <= kRsMaxIn, "RsRestoreDesc::out holds a repair's outputs");

// What restore_plan and repair_plan make of one pattern.
struct RsPlan {
    int inputs[kRsMaxIn];
    int outputs[kRsMaxOut];
    int nout = 0;
    uint8_t rows[kRsMaxOut * kRsMaxIn];   // nout x k
};
typedef RsPlan RestorePlan, RepairPlan;   // the names the two sides had before they shared the type

// The plan of one pattern: every data fragment that is missing or not at its final address is
// written, fragment j with row j of the inverse of the inputs' sub-matrix (a unit row when j is
// itself an input: a present data fragment always is).  in_place is nullable (nothing in place).
// Returns as rs_pick_inputs.
inline int restore_plan(const uint8_t* mat, int k, int m, const uint8_t* present, const uint8_t* in_place, RsPlan& p) {
    uint8_t inv[kRsMaxIn * kRsMaxIn];
    const int got = rs_pick_inputs(mat, k, m, present, p.inputs, inv);
    if (got != k) return got;
    p.nout = 0;
    for (int j = 0; j < k; j++) {
        if (present[j] && in_place && in_place[j]) continue;
        p.outputs[p.nout] = j;
        std::memcpy(p.rows + p.nout * k, inv + j * k, (size_t)k);
        p.nout++;
    }
    return k;
}

enum : uint8_t { kFragAbsent = 0, kFragUsed = 1, kFragSpare = 2, kFragBad = 3 };
enum : uint8_t { kSegOk = 0, kSegTooFew = 1, kSegMismatch = 2, kSegBadPadding = 3 };

// Fragment states of ns segments -> statuses: the first k good fragments of a segment are used, the
// other good ones spare; a segment with fewer than k good ones is kSegTooFew (its good fragments
// stay spare: nothing is rebuilt from them).  `good` holds the address of a fragment that is on the
// device and passed its check, else null.  Returns false when any segment has too few.
inline bool rt_select(int k, int total, uint64_t ns, const uint8_t* const* good, uint8_t* fst, uint8_t* sst) {
    bool all = true;
    for (uint64_t t = 0; t < ns; t++) {
        int ng = 0;
        for (int j = 0; j < total; j++) ng += good[t * total + j] != nullptr;
        const bool enough = ng >= k;
        if (!enough) {
            sst[t] = kSegTooFew;
            all = false;
        }
        int used = 0;
        for (int j = 0; j < total; j++)
            if (good[t * total + j]) fst[t * total + j] = (enough && used++ < k) ? kFragUsed : kFragSpare;
    }
    return all;
}

// The plan of one pattern for a repair: every fragment j with want[j] && !present[j] is written (want
// nullable: every missing one), a data fragment with row j of the inverse of the inputs' sub-matrix,
// a parity fragment with mat[j] x that inverse.  A present fragment is never written.  At most
// m <= kRsMaxOut fragments are missing once k are present.  Returns as rs_pick_inputs.
inline int repair_plan(const uint8_t* mat, int k, int m, const uint8_t* present, const uint8_t* want, RsPlan& p) {
    uint8_t inv[kRsMaxIn * kRsMaxIn];
    const int got = rs_pick_inputs(mat, k, m, present, p.inputs, inv);
    if (got != k) return got;
    const Gf& g = gf();
    p.nout = 0;
    for (int j = 0; j < k + m; j++) {
        if (present[j] || (want && !want[j])) continue;
        uint8_t* row = p.rows + p.nout * k;
        if (j < k) {
            std::memcpy(row, inv + j * k, (size_t)k);
        } else {
            const uint8_t* mrow = mat + j * k;   // output = mrow x data = mrow x inv x inputs
            for (int c = 0; c < k; c++) {
                uint8_t acc = 0;
                for (int q = 0; q < k; q++) acc ^= g.mul(mrow[q], inv[q * k + c]);
                row[c] = acc;
            }
        }
        p.outputs[p.nout++] = j;
    }
    return k;
}

// Descriptors and coding tables of one restore or one repair launch, built segment by segment; mat
// is the coder's (k + m) x k matrix and outlives the batch.
struct RsBatch {
    struct Cached {
        RsPlan p;
        uint32_t tab;
    };
    const uint8_t* mat;
    int k, m;
    std::vector<dm::RsRestoreDesc> desc;
    std::vector<uint64_t> tabs;                 // [ntab][k][256]
    std::map<uint32_t, Cached> plans;           // present mask | in-place (restore) or want (repair) mask << 16
    std::map<std::string, uint32_t> tab_of;     // coding rows -> table index (one table per distinct plan)
    bool any_out = false;
    bool any_wide = false;                      // some segment has nout > k (repair only): rs_restore_kernel cannot run it
};
typedef RsBatch RestoreBatch, RepairBatch;

// What restore_add and repair_add share once a segment's key is known: its plan (cached by key, else
// from plan(RsPlan&), which returns as rs_pick_inputs), the plan's table (shared by coding rows), and
// the descriptor, whose inputs are frags[plan input] and whose output i lies at out_at(fragment index).
template <class PlanFn, class OutFn>
inline int batch_add(RsBatch& b, uint32_t key, const uint8_t* const* frags, PlanFn plan, OutFn out_at) {
    const int k = b.k;
    auto it = b.plans.find(key);
    if (it == b.plans.end()) {
        RsBatch::Cached cp;
        const int got = plan(cp.p);
        if (got != k) return got;
        cp.tab = 0;
        if (cp.p.nout) {
            const std::string rows(reinterpret_cast<const char*>(cp.p.rows), (size_t)cp.p.nout * k);
            auto t = b.tab_of.find(rows);
            if (t == b.tab_of.end()) {
                const std::vector<uint64_t> tab = rs_table(cp.p.rows, cp.p.nout, k);
                t = b.tab_of.emplace(rows, (uint32_t)(b.tabs.size() / ((size_t)k * 256))).first;
                b.tabs.insert(b.tabs.end(), tab.begin(), tab.end());
            }
            cp.tab = t->second;
        }
        it = b.plans.emplace(key, cp).first;
    }
    const RsPlan& p = it->second.p;
    dm::RsRestoreDesc ds{};
    for (int j = 0; j < k; j++) ds.in[j] = frags[p.inputs[j]];
    for (int i = 0; i < p.nout; i++) ds.out[i] = out_at(p.outputs[i]);
    ds.nout = (uint32_t)p.nout;
    ds.table = it->second.tab;
    if (p.nout) b.any_out = true;
    if (p.nout > k) b.any_wide = true;
    b.desc.push_back(ds);
    return k;
}

// Segment whose usable fragments are frags[0 .. total) (device addresses, NULL = absent; never
// dereferenced here) and whose data fragment j belongs at seg_base + j * frag.  Returns as
// rs_pick_inputs.
inline int restore_add(RestoreBatch& b, const uint8_t* const* frags, uint8_t* seg_base, uint64_t frag) {
    const int k = b.k, total = b.k + b.m;
    uint8_t present[kRsMaxIn + kRsMaxOut], in_place[kRsMaxIn];
    uint32_t key = 0;
    for (int j = 0; j < total; j++) {
        present[j] = frags[j] != nullptr;
        key |= (uint32_t)present[j] << j;
        if (j < k) {
            in_place[j] = frags[j] == seg_base + (uint64_t)j * frag;
            key |= (uint32_t)in_place[j] << (16 + j);
        }
    }
    return batch_add(b, key, frags, [&](RsPlan& p) { return restore_plan(b.mat, k, b.m, present, in_place, p); },
                     [&](int j) { return seg_base + (uint64_t)j * frag; });
}

// Segment whose fragment j lies, or is to be written, at frags[j] (device addresses, never
// dereferenced here): present[j] != 0 holds the fragment; present[j] == 0 and frags[j] != NULL is
// wanted; NULL is absent and not wanted.  Returns as rs_pick_inputs.
inline int repair_add(RepairBatch& b, uint8_t* const* frags, const uint8_t* present) {
    const int total = b.k + b.m;
    uint8_t pres[kRsMaxIn + kRsMaxOut], want[kRsMaxIn + kRsMaxOut];
    uint32_t key = 0;
    for (int j = 0; j < total; j++) {
        pres[j] = present[j] != 0 && frags[j] != nullptr;
        want[j] = !pres[j] && frags[j] != nullptr;
        key |= (uint32_t)pres[j] << j | (uint32_t)want[j] << (16 + j);
    }
    return batch_add(b, key, frags, [&](RsPlan& p) { return repair_plan(b.mat, b.k, b.m, pres, want, p); },
                     [&](int j) { return frags[j]; });
}

// ---- any geometry up to 256 shards: the standalone coder (dm_rs_create_wide) --------------------
// Heap-backed forms of the inverse, the matrix and the reconstruct plan for any k <= 255, and the
// table layout of rs_code_wide_kernel.  Same arithmetic and pivoting as the fixed-size forms above,
// so within 8 + 8 they give the same bytes.

constexpr int kRsWideMaxShards = 256;   // klauspost: data + parity <= 256
constexpr int kRsGroup = 8;             // outputs per table entry (one byte each)
constexpr int kRsWideEntries = 32;      // table entries per input and group: 16 low-nibble, 16 high-nibble

// Gauss-Jordan inverse of a k x k GF(2^8) matrix, any k; false if singular.
inline bool gf_invert_n(const uint8_t* m, int k, std::vector<uint8_t>& out) {
    const Gf& g = gf();
    const size_t w2 = 2 * (size_t)k;
    std::vector<uint8_t> w((size_t)k * w2, 0);
    for (int r = 0; r < k; r++) {
        std::memcpy(&w[r * w2], m + (size_t)r * k, (size_t)k);
        w[r * w2 + k + r] = 1;
    }
    for (int c = 0; c < k; c++) {
        int p = c;
        while (p < k && w[p * w2 + c] == 0) p++;
        if (p == k) return false;
        if (p != c) std::swap_ranges(&w[p * w2], &w[p * w2] + w2, &w[c * w2]);
        uint8_t* pc = &w[c * w2];
        const uint8_t s = g.inv(pc[c]);
        for (size_t j = 0; j < w2; j++) pc[j] = g.mul(pc[j], s);
        for (int r = 0; r < k; r++) {
            uint8_t* pr = &w[r * w2];
            if (r == c || pr[c] == 0) continue;
            const uint8_t f = pr[c];
            for (size_t j = 0; j < w2; j++) pr[j] ^= g.mul(f, pc[j]);
        }
    }
    out.resize((size_t)k * k);
    for (int r = 0; r < k; r++) std::memcpy(&out[(size_t)r * k], &w[r * w2 + k], (size_t)k);
    return true;
}

// rows (n x k) x b (k x k) -> out (n x k).
inline void gf_matmul_n(const uint8_t* rows, int n, const uint8_t* b, int k, uint8_t* out) {
    const Gf& g = gf();
    for (int i = 0; i < n; i++) {
        uint8_t* o = out + (size_t)i * k;
        std::memset(o, 0, (size_t)k);
        for (int t = 0; t < k; t++) {
            const uint8_t f = rows[(size_t)i * k + t];
            if (!f) continue;
            const uint8_t* br = b + (size_t)t * k;
            for (int j = 0; j < k; j++) o[j] ^= g.mul(f, br[j]);
        }
    }
}

// rs_build_matrix for 1 <= k, 1 <= m, k + m <= 256.
inline bool rs_build_matrix_n(int k, int m, std::vector<uint8_t>& mat) {
    const Gf& g = gf();
    const int total = k + m;
    std::vector<uint8_t> vm((size_t)total * k);
    for (int i = 0; i < total; i++)
        for (int j = 0; j < k; j++) vm[(size_t)i * k + j] = g.pow((uint8_t)i, j);
    std::vector<uint8_t> inv;
    if (!gf_invert_n(vm.data(), k, inv)) return false;
    mat.assign((size_t)total * k, 0);
    gf_matmul_n(vm.data(), total, inv.data(), k, mat.data());
    return true;
}

struct ReconstructPlan {
    std::vector<int> inputs;     // k: the first k present shards in index order
    std::vector<int> outputs;    // every shard that is not present, in index order
    std::vector<uint8_t> rows;   // outputs.size() x k
};

// klauspost's Reconstruct for one pattern (present[k + m]): a missing data shard gets its row of the
// inverse of the inputs' sub-matrix, a missing parity shard (parity row) x that inverse.  Returns as
// rs_pick_inputs; with nothing missing the plan has no outputs and nothing is inverted.
inline int reconstruct_plan(const uint8_t* mat, int k, int m, const uint8_t* present, ReconstructPlan& p) {
    const int total = k + m;
    p.inputs.clear();
    p.outputs.clear();
    p.rows.clear();
    int nv = 0;
    for (int i = 0; i < total; i++) {
        if (!present[i]) p.outputs.push_back(i);
        else if (nv++ < k) p.inputs.push_back(i);
    }
    if (nv < k) return nv;
    if (p.outputs.empty()) return k;
    std::vector<uint8_t> sub((size_t)k * k), inv;
    for (int i = 0; i < k; i++) std::memcpy(&sub[(size_t)i * k], mat + (size_t)p.inputs[i] * k, (size_t)k);
    if (!gf_invert_n(sub.data(), k, inv)) return kPlanSingular;
    p.rows.resize(p.outputs.size() * (size_t)k);
    for (size_t t = 0; t < p.outputs.size(); t++) {
        const int o = p.outputs[t];
        uint8_t* row = &p.rows[t * (size_t)k];
        if (o < k) std::memcpy(row, &inv[(size_t)o * k], (size_t)k);
        else gf_matmul_n(mat + (size_t)o * k, 1, inv.data(), k, row);   // output = mrow x data = mrow x inv x inputs
    }
    return k;
}

// rs_code_wide_kernel's table of `rows` (nout x k, row-major): [ceil(nout / 8)][k][32] entries of
// 8 B.  For output group g and input j, byte i of entry n < 16 is rows[8g + i][j] * n (the low
// nibble's product) and of entry 16 + n is rows[8g + i][j] * (n << 4) (the high nibble's); a byte
// past the last output is 0.  x * c = (x & 15) * c ^ (x & 0xf0) * c.
inline std::vector<uint64_t> rs_wide_table(const uint8_t* rows, int nout, int k) {
    const Gf& g = gf();
    const int groups = (nout + kRsGroup - 1) / kRsGroup;
    std::vector<uint64_t> t((size_t)groups * k * kRsWideEntries, 0);
    for (int gr = 0; gr < groups; gr++)
        for (int j = 0; j < k; j++)
            for (int n = 0; n < kRsWideEntries; n++) {
                const uint8_t x = n < 16 ? (uint8_t)n : (uint8_t)((n - 16) << 4);
                uint64_t e = 0;
                for (int i = 0; i < kRsGroup && gr * kRsGroup + i < nout; i++)
                    e |= (uint64_t)g.mul(rows[(size_t)(gr * kRsGroup + i) * k + j], x) << (8 * i);
                t[((size_t)gr * k + j) * kRsWideEntries + n] = e;
            }
    return t;
}

}  // namespace dm_rsplan
