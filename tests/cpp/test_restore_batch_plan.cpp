// Host test of the batched restore's plan (deoss_amd/csrc/restore_batch_plan.hpp), stepped alone:
// object counts {0, 1, 2, 17}, nseg {1, 2, 5}, parity fragments given {0, 1, 8} per segment, ciphers
// {none, 16, 24, 32 bytes, two objects sharing one cipher}, objects marked failed before the decrypt
// stage.  Offsets are 16-byte aligned and disjoint, the totals match, the chain list holds exactly
// the surviving encrypted segments, keys are deduplicated, and every argument error names the right
// object.  No GPU.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../deoss_amd/csrc/restore_batch_plan.hpp"

namespace rp = dm_restore_plan;

static int failures = 0;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
            failures++;                                    \
        }                                                  \
    } while (0)

constexpr int K = 4, M = 8, TOTAL = K + M;
constexpr uint64_t SEG = 256, FRAG = SEG / K, PIECE = SEG - 16;

static const uint64_t kNseg[3] = {1, 2, 5};
static const int kPar[3] = {0, 1, 8};

// The objects of a case own their pointer tables and cipher bytes.
struct Batch {
    std::vector<std::vector<const void*>> frags;
    std::vector<std::vector<uint8_t>> ciphers;
    std::vector<rp::Obj> objs;
};

static char g_frag;   // what a present fragment points at: the plan only tests for null
static char g_out;

// cipher kind of object o: 0 none, 1/2/3 = 16/24/32 bytes of its own, 4 = the bytes of the previous
// encrypted object (in another buffer: shared by value, not by pointer).
static Batch make(uint64_t nobj, int a, int b, int c) {
    Batch B;
    B.frags.resize(nobj);
    B.ciphers.resize(nobj);
    B.objs.resize(nobj);
    int last_enc = -1;
    for (uint64_t o = 0; o < nobj; o++) {
        const uint64_t nseg = kNseg[(o + a) % 3];
        const int par = kPar[(o + b) % 3];
        B.frags[o].assign(nseg * TOTAL, nullptr);
        for (uint64_t t = 0; t < nseg; t++) {
            for (int j = 0; j < K; j++)
                if ((o + t + j) % 3) B.frags[o][t * TOTAL + j] = &g_frag;   // some data fragments missing
            for (int j = 0; j < par; j++) B.frags[o][t * TOTAL + K + (j * 5 + (int)t) % M] = &g_frag;
        }
        int kind = (int)((o + c) % 5);
        if (kind == 4 && last_enc < 0) kind = 2;
        if (kind == 4) {
            B.ciphers[o] = B.ciphers[last_enc];
        } else if (kind) {
            B.ciphers[o].resize(8 + 8 * kind);
            for (size_t i = 0; i < B.ciphers[o].size(); i++) B.ciphers[o][i] = (uint8_t)(o * 37 + i * 11 + 1);
        }
        if (kind) last_enc = (int)o;
        rp::Obj& x = B.objs[o];
        x.frags = B.frags[o].data();
        x.nseg = nseg;
        x.cipher = kind ? B.ciphers[o].data() : nullptr;
        x.cipher_len = B.ciphers[o].size();
        x.size = (nseg - 1) * (kind ? PIECE : SEG) + 1 + (o * 7) % (kind ? PIECE : SEG);
        x.out = &g_out;
    }
    return B;
}

struct Span {
    uint64_t lo, hi;
    const char* what;
    uint64_t obj;
};

static void check_disjoint(std::vector<Span> v, uint64_t limit, const char* buf) {
    std::sort(v.begin(), v.end(), [](const Span& x, const Span& y) { return x.lo < y.lo; });
    for (size_t i = 0; i < v.size(); i++) {
        CHECK(v[i].hi <= limit, "%s: %s of object %llu ends at %llu beyond %llu", buf, v[i].what,
              (unsigned long long)v[i].obj, (unsigned long long)v[i].hi, (unsigned long long)limit);
        if (i) CHECK(v[i - 1].hi <= v[i].lo, "%s: %s of object %llu overlaps %s of object %llu", buf, v[i - 1].what,
                     (unsigned long long)v[i - 1].obj, v[i].what, (unsigned long long)v[i].obj);
    }
}

static void check_case(uint64_t nobj, int a, int b, int c) {
    const Batch B = make(nobj, a, b, c);
    const rp::Error e = rp::check(B.objs.data(), nobj, SEG, K);
    CHECK(!e, "valid batch refused: %s", e.msg.c_str());
    const rp::Plan p = rp::plan(B.objs.data(), nobj, SEG, K, M);
    CHECK(p.obj.size() == nobj && p.frag == FRAG && p.piece == PIECE && p.total == TOTAL, "shape");
    uint64_t nseg = 0, npar = 0, enc = 0;
    std::vector<Span> data, work;
    std::set<std::string> distinct;
    for (uint64_t o = 0; o < nobj; o++) {
        const rp::Obj& x = B.objs[o];
        const rp::ObjPlan& q = p.obj[o];
        uint64_t par = 0;
        for (uint64_t t = 0; t < x.nseg; t++)
            for (int j = K; j < TOTAL; j++) par += x.frags[t * TOTAL + j] != nullptr;
        CHECK(q.seg0 == nseg, "object %llu: seg0 %llu, want %llu", (unsigned long long)o, (unsigned long long)q.seg0,
              (unsigned long long)nseg);
        CHECK(q.obj_off == nseg * SEG, "object %llu: obj_off", (unsigned long long)o);
        CHECK(q.npar == par, "object %llu: npar %llu, want %llu", (unsigned long long)o, (unsigned long long)q.npar,
              (unsigned long long)par);
        CHECK(q.obj_off % 16 == 0 && q.par_off % 16 == 0 && q.fid_off % 16 == 0, "object %llu: alignment", (unsigned long long)o);
        data.push_back({q.obj_off, q.obj_off + x.nseg * SEG, "segments", o});
        if (par) work.push_back({q.par_off, q.par_off + par * FRAG, "parity slots", o});
        work.push_back({q.fid_off, q.fid_off + 32, "fid", o});
        if (x.encrypted()) {
            CHECK(q.key >= 0 && (size_t)q.key < p.keys.size(), "object %llu: key %d", (unsigned long long)o, q.key);
            if (q.key >= 0 && (size_t)q.key < p.keys.size()) {
                const rp::KeyRef& kr = p.keys[q.key];
                CHECK(kr.len == x.cipher_len && std::memcmp(kr.bytes, x.cipher, x.cipher_len) == 0,
                      "object %llu: key entry %d holds other bytes", (unsigned long long)o, q.key);
            }
            distinct.insert(std::string(static_cast<const char*>(x.cipher), x.cipher_len));
            CHECK(q.plain_off % 16 == 0, "object %llu: plain_off %llu", (unsigned long long)o, (unsigned long long)q.plain_off);
            work.push_back({q.plain_off, q.plain_off + x.nseg * PIECE, "plaintext", o});
            work.push_back({q.pad_off, q.pad_off + x.nseg, "verdicts", o});
            CHECK(q.pad_off == p.pad_base + enc, "object %llu: pad_off", (unsigned long long)o);
            enc += x.nseg;
        } else {
            CHECK(q.key == -1, "object %llu: plain object has key %d", (unsigned long long)o, q.key);
        }
        nseg += x.nseg;
        npar += par;
    }
    CHECK(p.nseg == nseg && p.npar == npar && p.enc_nseg == enc, "totals: %llu %llu %llu", (unsigned long long)p.nseg,
          (unsigned long long)p.npar, (unsigned long long)p.enc_nseg);
    CHECK(p.keys.size() == distinct.size(), "%zu key entries for %zu distinct ciphers", p.keys.size(), distinct.size());
    CHECK(p.plain_base % 16 == 0 && p.pad_base % 16 == 0 && p.fid_base % 16 == 0, "region bases");
    CHECK(p.data_bytes >= nseg * SEG && p.device_bytes() == p.data_bytes + p.work_bytes, "device bytes");
    check_disjoint(data, p.data_bytes, "object buffer");
    check_disjoint(work, p.work_bytes, "scratch");
    // the chain list under three sets of survivors: all, all but every third object, none
    for (int mode = 0; mode < 3; mode++) {
        std::vector<uint8_t> alive(nobj);
        for (uint64_t o = 0; o < nobj; o++) alive[o] = mode == 0 ? 1 : mode == 1 ? (o + a) % 3 != 0 : 0;
        std::vector<uint64_t> chain0;
        const std::vector<rp::Chain> ch = rp::decrypt_chains(p, B.objs.data(), alive.data(), &chain0);
        size_t at = 0;
        for (uint64_t o = 0; o < nobj; o++) {
            if (!B.objs[o].encrypted() || !alive[o]) continue;
            CHECK(chain0[o] == at, "mode %d: chain0 of object %llu", mode, (unsigned long long)o);
            for (uint64_t t = 0; t < B.objs[o].nseg; t++, at++) {
                CHECK(at < ch.size(), "mode %d: chain list too short", mode);
                if (at >= ch.size()) return;
                const rp::Chain& x = ch[at];
                CHECK(x.obj == o && x.seg == t && x.in_off == p.obj[o].obj_off + t * SEG &&
                          x.out_off == p.obj[o].plain_off + t * PIECE && (int32_t)x.key == p.obj[o].key,
                      "mode %d: chain %zu is not segment %llu of object %llu", mode, at, (unsigned long long)t,
                      (unsigned long long)o);
            }
        }
        CHECK(at == ch.size(), "mode %d: %zu chains, want %zu", mode, ch.size(), at);
    }
}

// Object `bad` of a valid batch of n broken in every way: the error names it, whatever comes after.
static void check_errors(uint64_t n, uint64_t bad) {
    const uint8_t short_key[15] = {1};
    for (int way = 0; way < 7; way++) {
        Batch B = make(n, 1, 2, 1);
        rp::Obj& x = B.objs[bad];
        if (bad + 1 < n) B.objs[bad + 1].nseg = 0;   // a later error must not be the one reported
        const uint64_t piece = x.encrypted() ? PIECE : SEG;
        rp::Code want = rp::kInvalid;
        const char* text = "";
        switch (way) {
            case 0: x.nseg = 0; want = rp::kEmpty; text = "Empty data"; break;
            case 1: x.size = x.nseg * piece + 1; text = "does not end in the last of"; break;
            case 2: x.size = (x.nseg - 1) * piece; text = "does not end in the last of"; break;
            case 3: x.cipher = short_key; x.cipher_len = 15; text = "cipher must be 16, 24 or 32 bytes"; break;
            case 4: x.cipher = short_key; x.cipher_len = 33; text = "cipher must be 16, 24 or 32 bytes"; break;
            case 5: x.frags = nullptr; text = "null argument"; break;
            case 6: x.out = nullptr; text = "null argument"; break;
        }
        const rp::Error e = rp::check(B.objs.data(), n, SEG, K);
        const std::string who = "bject " + std::to_string(bad);
        CHECK(e.code == want && e.obj == bad, "way %d at object %llu: code %d, object %llu", way, (unsigned long long)bad,
              (int)e.code, (unsigned long long)e.obj);
        CHECK(e.msg.find(who) != std::string::npos && e.msg.find(text) != std::string::npos, "way %d at object %llu: \"%s\"",
              way, (unsigned long long)bad, e.msg.c_str());
    }
}

int main() {
    const uint64_t counts[] = {0, 1, 2, 17};
    int cases = 0;
    for (uint64_t n : counts)
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++)
                for (int c = 0; c < 5; c++) {
                    check_case(n, a, b, c);
                    cases++;
                }
    for (uint64_t bad : {0, 1, 9, 16}) check_errors(17, bad);
    check_errors(1, 0);
    // no objects: an empty plan that still has its slack
    const rp::Plan none = rp::plan(nullptr, 0, SEG, K, M);
    CHECK(none.nseg == 0 && none.keys.empty() && none.obj.empty(), "empty plan");
    CHECK(rp::decrypt_chains(none, nullptr, nullptr).empty(), "chains of no objects");
    // the segment size: a multiple of 16 x data shards (batch-wide), and room for a padding block
    // only where an object has a cipher -- 16-byte segments at one data shard serve plain objects
    CHECK(rp::check(nullptr, 0, 100, K).code == rp::kInvalid && rp::check(nullptr, 0, 0, K).code == rp::kInvalid, "segment size");
    {
        const void* f[2] = {&g_frag, nullptr};
        const uint8_t key[16] = {7};
        rp::Obj two[2];
        two[0].frags = two[1].frags = f;
        two[0].nseg = two[1].nseg = 1;
        two[0].size = two[1].size = 16;
        two[0].out = two[1].out = &g_out;
        CHECK(!rp::check(two, 2, 16, 1), "plain objects at 16-byte segments");
        two[1].cipher = key;
        two[1].cipher_len = 16;
        const rp::Error e = rp::check(two, 2, 16, 1);
        CHECK(e.code == rp::kInvalid && e.obj == 1 && e.msg.find("object 1") != std::string::npos &&
                  e.msg.find("no room for a block and its padding block") != std::string::npos,
              "cipher at 16-byte segments: \"%s\"", e.msg.c_str());
        // a cipher pointer with length 0, or a length without a pointer, is a plain object
        two[1].cipher_len = 0;
        CHECK(!rp::check(two, 2, 16, 1), "cipher_len 0");
        two[1].cipher = nullptr;
        two[1].cipher_len = 16;
        CHECK(!rp::check(two, 2, 16, 1), "null cipher");
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("restore batch plan OK (%d cases)\n", cases);
    return 0;
}
