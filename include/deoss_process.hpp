// deoss_process.hpp -- C++ host mirror of the Go process shim (go/process): cess-go-sdk
// process.FullProcessing(file, cipher, savedir) (go.mod:8; node/objectHandler.go:168,
// node/fileHandler.go:771, node/filesHandler.go:201, node/resumeHandler.go:326,
// node/tracker.go:767-769) and the streaming Writer (go/process/stream_hip.go), over the C ABI
// (include/deoss_merkle.h: dm_full_processing, dm_pstream_*).  Same result shape: segment and
// fragment path names under savedir (every one exists as a file), the hex fid, an error.
// A non-empty cipher takes the same one call (dm_full_processing_cipher; the scheme is recalled
// from the SDK, parity-unpinned: DESIGN.md §6.14; the Go shim still routes a cipher to the SDK).
// Header-only; link -ldeoss_merkle.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <optional>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include <sys/stat.h>

#include "deoss_merkle.h"

namespace process {

constexpr uint64_t SegmentSize = 32ull << 20;   // chain.SegmentSize
constexpr int DataShards = 4, ParShards = 8;    // chain.DataShards / chain.ParShards

struct Error {
    int code;
    std::string message;
};

struct SegmentDataInfo {   // chain.SegmentDataInfo
    std::string SegmentHash;
    std::vector<std::string> FragmentHash;
};

using Result = std::tuple<std::vector<SegmentDataInfo>, std::string, std::optional<Error>>;

// One coder per visible GPU, created on first use; calls pick one round robin (each call holds
// its coder's context for its duration, so concurrent calls spread over the GPUs).
class Pipelines {
  public:
    static Pipelines& instance() {
        static Pipelines p;
        return p;
    }
    dm_rs* pick() { return rs_.empty() ? nullptr : rs_[next_++ % rs_.size()]; }
    // a coder and the context it lives on (the cipher window path reduces the fid on it)
    std::pair<dm_rs*, dm_ctx*> pick_pair() {
        if (rs_.empty()) return {nullptr, nullptr};
        const size_t i = next_++ % rs_.size();
        return {rs_[i], ctx_[i]};
    }
    int status() const { return rc_; }
    ~Pipelines() {
        for (dm_rs* r : rs_) dm_rs_destroy(r);
        for (dm_ctx* c : ctx_) dm_destroy(c);
    }

  private:
    Pipelines() {
        const int n = dm_gpu_count();
        if (n <= 0) rc_ = DM_ERR_NODEV;
        for (int g = 0; g < n && rc_ == DM_OK; g++) {
            dm_ctx* c = nullptr;
            dm_rs* r = nullptr;
            if ((rc_ = dm_create(&c, &g, 1)) != DM_OK) break;
            ctx_.push_back(c);
            if ((rc_ = dm_rs_create(c, DataShards, ParShards, &r)) != DM_OK) break;
            rs_.push_back(r);
        }
    }
    std::vector<dm_ctx*> ctx_;
    std::vector<dm_rs*> rs_;
    std::atomic<uint64_t> next_{0};
    int rc_ = DM_OK;
};

inline bool write_segments() {
    const char* v = std::getenv("DEOSS_SKIP_SEGMENT_FILES");
    return !(v && v[0] == '1' && v[1] == 0);
}

inline Error last_error(int rc) {   // dm_last_error is the calling thread's message
    if (rc == DM_ERR_EMPTY) return {rc, "Empty data"};
    std::string m = dm_last_error(nullptr);
    return {rc, m.empty() ? std::string(dm_strerror(rc)) : m};
}

inline std::string hex32(const uint8_t* d) {
    static const char* x = "0123456789abcdef";
    std::string s(64, '0');
    for (int i = 0; i < 32; i++) {
        s[2 * i] = x[d[i] >> 4];
        s[2 * i + 1] = x[d[i] & 15];
    }
    return s;
}

inline std::string join(const std::string& dir, const std::string& name) {
    return dir.empty() || dir.back() == '/' ? dir + name : dir + "/" + name;
}

inline std::vector<SegmentDataInfo> infos(const std::string& savedir, const std::vector<uint8_t>& segd,
                                          const std::vector<uint8_t>& fragd, uint64_t nseg) {
    const int total = DataShards + ParShards;
    std::vector<SegmentDataInfo> out(nseg);
    for (uint64_t s = 0; s < nseg; s++) {
        out[s].SegmentHash = join(savedir, hex32(segd.data() + 32 * s));
        for (int j = 0; j < total; j++) out[s].FragmentHash.push_back(join(savedir, hex32(fragd.data() + 32 * (s * total + j))));
    }
    return out;
}

constexpr uint64_t WindowSegments = 8;   // segments per dm_process_cipher_buffer call (the cipher window path)

inline std::optional<Error> write_new(const std::string& path, const uint8_t* p, uint64_t n) {
    if (FILE* have = std::fopen(path.c_str(), "rb")) {   // named by content: an existing file is this one
        std::fclose(have);
        return std::nullopt;
    }
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return Error{DM_ERR_IO, "open " + path + ": cannot create"};
    const bool ok = std::fwrite(p, 1, n, f) == n;
    if (std::fclose(f) != 0 || !ok) return Error{DM_ERR_IO, "write " + path + ": short write"};
    return std::nullopt;
}

// FullProcessing(file, cipher != "", savedir) as it ran before dm_full_processing_cipher: the
// window path, kept callable as the A/B baseline.  The file is read in windows of
// WindowSegments pieces of segment - 16 plaintext bytes; each window is one
// dm_process_cipher_buffer call (AES-CBC, coding and names on the GPU; segments are independent
// chains, so windows carry no state), its fragment and segment files are written, and the fid is
// the tree over all segment digests.  PARITY-UNPINNED: the scheme is recalled from the SDK
// (deoss_merkle.h).  `segment` is chain.SegmentSize outside tests.
inline Result FullProcessingCipher(const std::string& file, const std::string& cipher, const std::string& savedir,
                                   uint64_t segment = SegmentSize) {
    auto& p = Pipelines::instance();
    auto [rs, ctx] = p.pick_pair();
    if (!rs) return {{}, "", Error{p.status(), dm_strerror(p.status())}};
    if (segment <= 16) return {{}, "", Error{DM_ERR_INVALID, "process: segment too small for a cipher"}};
    FILE* f = std::fopen(file.c_str(), "rb");
    if (!f) return {{}, "", Error{DM_ERR_IO, "open " + file + ": no such file or directory"}};
    (void)::mkdir(savedir.c_str(), 0777);   // as the library's file path: savedir may not exist yet
    const int total = DataShards + ParShards;
    const uint64_t piece = segment - 16, frag = segment / DataShards, window = WindowSegments * piece;
    const bool segfiles = write_segments();
    std::vector<uint8_t> buf(window), segd_all, fragd_all, frags;
    std::optional<Error> err;
    uint8_t fid[32] = {};
    uint64_t nseg_all = 0, calls = 0;
    for (;;) {
        const uint64_t got = std::fread(buf.data(), 1, window, f);
        if (got == 0) break;
        const uint64_t ns = (got + piece - 1) / piece;
        segd_all.resize(32 * (nseg_all + ns));
        fragd_all.resize(32 * (nseg_all + ns) * total);
        frags.resize(ns * total * frag);
        uint8_t* segd = segd_all.data() + 32 * nseg_all;
        uint8_t* fragd = fragd_all.data() + 32 * nseg_all * total;
        const int rc = dm_process_cipher_buffer(rs, buf.data(), got, segment, cipher.data(), cipher.size(), frags.data(),
                                                segd, fragd, fid);
        if (rc != DM_OK) {
            err = last_error(rc);
            break;
        }
        calls++;
        for (uint64_t s = 0; s < ns && !err; s++) {
            for (int j = 0; j < total && !err; j++)
                err = write_new(join(savedir, hex32(fragd + 32 * (s * total + j))), frags.data() + (s * total + j) * frag, frag);
            // data fragments in order = the segment's ciphertext
            if (segfiles && !err) err = write_new(join(savedir, hex32(segd + 32 * s)), frags.data() + s * total * frag, segment);
        }
        nseg_all += ns;
        if (err || got < window) break;
    }
    std::fclose(f);
    if (err) return {{}, "", err};
    if (nseg_all == 0) return {{}, "", Error{DM_ERR_EMPTY, "Empty data"}};
    if (calls > 1) {   // several windows: the tree over all segment digests
        std::vector<uint8_t> nodes(32 * dm_tree_node_count(nseg_all));
        const int rc = dm_tree_levels(ctx, segd_all.data(), nseg_all, nodes.data());
        if (rc != DM_OK) return {{}, "", last_error(rc)};
        std::copy(nodes.end() - 32, nodes.end(), fid);
    }
    return {infos(savedir, segd_all, fragd_all, nseg_all), hex32(fid), std::nullopt};
}

// The batch form: objects in memory, a cipher each ("" = a plain object of the same batch), ONE
// dm_process_cipher_batch call -- every encrypted object's pieces in one keyed AES-CBC launch
// whatever the mix of keys, then every segment coded and named in one pass.  What a handler that
// already holds several small encrypted uploads calls; concurrent handlers with one upload each
// take dm_batcher_process_cipher.  Per object: the segment digests, the fragment digests, the hex
// fid and (want_frags) the fragments, segment-major, data fragments first -- the outputs of
// dm_process_cipher_buffer / dm_process_buffer of the object alone.  PARITY-UNPINNED as above.
struct BatchObject {
    const void* data = nullptr;
    uint64_t len = 0;
    std::string cipher;
};

struct BatchOutput {
    std::vector<uint8_t> seg_hashes, frag_hashes, frags;
    std::string fid;
};

using BatchResult = std::pair<std::vector<BatchOutput>, std::optional<Error>>;

inline BatchResult FullProcessingCipherBatch(const std::vector<BatchObject>& objs, bool want_frags = true,
                                             uint64_t segment = SegmentSize) {
    auto& p = Pipelines::instance();
    dm_rs* rs = p.pick();
    if (!rs) return {{}, Error{p.status(), dm_strerror(p.status())}};
    const uint64_t n = objs.size(), total = DataShards + ParShards;
    if (segment <= 16) return {{}, Error{DM_ERR_INVALID, "process: segment too small for a cipher"}};
    std::vector<BatchOutput> out(n);
    std::vector<const void*> ptrs(n), keys(n);
    std::vector<uint64_t> lens(n), key_lens(n);
    std::vector<void*> fr(n);
    std::vector<uint8_t*> sh(n), fh(n);
    std::vector<uint8_t> fids(32 * n);
    for (uint64_t o = 0; o < n; o++) {
        const uint64_t piece = objs[o].cipher.empty() ? segment : segment - 16;
        const uint64_t ns = (objs[o].len + piece - 1) / piece;
        ptrs[o] = objs[o].data;
        lens[o] = objs[o].len;
        keys[o] = objs[o].cipher.empty() ? nullptr : objs[o].cipher.data();
        key_lens[o] = objs[o].cipher.size();
        out[o].seg_hashes.resize(32 * ns);
        out[o].frag_hashes.resize(32 * ns * total);
        if (want_frags) out[o].frags.resize(ns * total * (segment / DataShards));
        sh[o] = out[o].seg_hashes.data();
        fh[o] = out[o].frag_hashes.data();
        fr[o] = want_frags ? out[o].frags.data() : nullptr;
    }
    const int rc = dm_process_cipher_batch(rs, ptrs.data(), lens.data(), keys.data(), key_lens.data(), n, segment, fr.data(),
                                           sh.data(), fh.data(), fids.data());
    if (rc != DM_OK) return {{}, last_error(rc)};
    for (uint64_t o = 0; o < n; o++) out[o].fid = hex32(fids.data() + 32 * o);
    return {std::move(out), std::nullopt};
}

// FullProcessing(file, cipher, savedir): one dm_full_processing call (the library reads the file
// and writes every fragment and segment file to savedir/<hex SHA-256>); with a cipher,
// dm_full_processing_cipher, the same call over segments of ciphertext.  `segment` is
// chain.SegmentSize outside tests.
inline Result FullProcessing(const std::string& file, const std::string& cipher, const std::string& savedir,
                             uint64_t segment = SegmentSize) {
    auto& p = Pipelines::instance();
    dm_rs* rs = p.pick();
    if (!rs) return {{}, "", Error{p.status(), dm_strerror(p.status())}};
    const int flags = write_segments() ? DM_FP_SEGMENT_FILES : 0;
    uint64_t cap = 1;
    for (int attempt = 0; attempt < 3; attempt++) {   // cap from the library's count when too small
        std::vector<uint8_t> segd(32 * cap), fragd(32 * cap * (DataShards + ParShards));
        uint8_t fid[32];
        uint64_t nseg = 0;
        const int rc = dm_full_processing_cipher(rs, file.c_str(), savedir.c_str(), segment, cipher.data(), cipher.size(),
                                                 flags, segd.data(), fragd.data(), cap, &nseg, fid);
        if (rc == DM_ERR_INVALID && nseg > cap) {
            cap = nseg;
            continue;
        }
        if (rc != DM_OK) return {{}, "", last_error(rc)};
        return {infos(savedir, segd, fragd, nseg), hex32(fid), std::nullopt};
    }
    return {{}, "", Error{DM_ERR_INVALID, "process: file size changed during the call"}};
}

// FindFragment(fpath, fragmentHash) (go/process: the download handler's one fragment,
// node/fileHandler.go:962-979): the fragment bytes, an empty vector when the file has no fragment
// of that name, or an error.  dm_fragment_lookup: nothing is written to disk.
inline std::pair<std::vector<uint8_t>, std::optional<Error>> FindFragment(const std::string& fpath,
                                                                          const std::string& fragment_hash) {
    // fragment files are named by lower-case hex SHA-256 and the handler compares strings
    // (node/fileHandler.go:968): any other spelling names no fragment (not found, no error)
    uint8_t want[32];
    auto nib = [](char ch) -> int { return ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1; };
    bool ok = fragment_hash.size() == 64;
    for (int i = 0; ok && i < 32; i++) {
        const int hi = nib(fragment_hash[2 * i]), lo = nib(fragment_hash[2 * i + 1]);
        ok = hi >= 0 && lo >= 0;
        want[i] = (uint8_t)(hi * 16 + lo);
    }
    if (!ok) return {{}, std::nullopt};
    auto& p = Pipelines::instance();
    dm_rs* rs = p.pick();
    if (!rs) return {{}, Error{p.status(), dm_strerror(p.status())}};
    std::vector<uint8_t> out(SegmentSize / DataShards);
    int found = 0, idx = 0;
    uint64_t seg = 0;
    const int rc = dm_fragment_lookup(rs, fpath.c_str(), SegmentSize, want, out.data(), out.size(), &found, &seg, &idx);
    if (rc != DM_OK) return {{}, last_error(rc)};
    if (!found) out.clear();
    return {std::move(out), std::nullopt};
}

// RestoreFile(fragDir, segs, size, outPath) (go/process/restore_hip.go): the RSRestore / join /
// truncate part of process.Retrievefile (node/fileHandler.go:519,600,990).  segs is what
// FullProcessing returned; whichever of its fragments lie in fragDir/<name> rebuild the file of
// `size` bytes at outPath.  dm_retrieve_file: every fragment used and every restored segment is
// checked against its name; outPath appears only when all held.
inline std::optional<Error> RestoreFile(const std::string& fragdir, const std::vector<SegmentDataInfo>& segs,
                                        uint64_t size, const std::string& out_path) {
    auto base32 = [](const std::string& path, uint8_t* out) -> bool {
        const std::string n = path.substr(path.rfind('/') == std::string::npos ? 0 : path.rfind('/') + 1);
        auto nib = [](char ch) -> int { return ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1; };
        if (n.size() != 64) return false;
        for (int i = 0; i < 32; i++) {
            const int hi = nib(n[2 * i]), lo = nib(n[2 * i + 1]);
            if (hi < 0 || lo < 0) return false;
            out[i] = (uint8_t)(hi * 16 + lo);
        }
        return true;
    };
    const int total = DataShards + ParShards;
    std::vector<uint8_t> segn(32 * segs.size()), fragn(32 * segs.size() * total), sst(segs.size());
    for (size_t s = 0; s < segs.size(); s++) {
        bool ok = (int)segs[s].FragmentHash.size() == total && base32(segs[s].SegmentHash, segn.data() + 32 * s);
        for (int j = 0; ok && j < total; j++) ok = base32(segs[s].FragmentHash[j], fragn.data() + 32 * (s * total + j));
        if (!ok) return Error{DM_ERR_INVALID, "process: segment and fragment names must be hex SHA-256"};
    }
    auto& p = Pipelines::instance();
    dm_rs* rs = p.pick();
    if (!rs) return Error{p.status(), dm_strerror(p.status())};
    int ok = 0;
    const int rc = dm_retrieve_file(rs, fragdir.c_str(), fragn.data(), segn.data(), nullptr, segs.size(), size, SegmentSize,
                                    DM_RESTORE_VERIFY_FRAGMENTS | DM_RESTORE_VERIFY_SEGMENTS, out_path.c_str(), nullptr,
                                    sst.data(), &ok);
    if (rc != DM_OK) return last_error(rc);
    if (!ok) return Error{DM_ERR_INVALID, "process: restore failed: too few verified fragments or a segment mismatch"};
    return std::nullopt;
}

// RestoreBatch (go/process/restore_hip.go RestoreBuffers, for a caller that already holds several
// downloads): many objects restored from fragments in memory and verified in ONE dm_restore_batch
// pass -- one staging, one leaf launch over the fragments, one restore launch, one leaf launch over
// the segments, one keyed decrypt launch whatever the mix of ciphers.  Per object what
// dm_restore_buffer / dm_restore_cipher_buffer give for it alone; an object that fails its checks
// has ok = false and no data, and changes nothing for the others.  Concurrent handlers with one
// download each take dm_batcher_restore.  With a cipher: PARITY-UNPINNED as above.
struct RestoreObject {
    std::vector<const void*> frags;                    // nseg x (data + parity), nullptr = not downloaded
    std::vector<uint8_t> frag_names, seg_names, fid;   // each may be empty: its check is skipped
    uint64_t size = 0;                                 // plaintext bytes when there is a cipher
    int flags = DM_RESTORE_VERIFY_ALL;
    std::string cipher;
};

struct RestoreOutput {
    bool ok = false;
    std::vector<uint8_t> data, frag_status, seg_status;
};

using RestoreBatchResult = std::pair<std::vector<RestoreOutput>, std::optional<Error>>;

inline RestoreBatchResult RestoreBatch(const std::vector<RestoreObject>& objs, uint64_t segment = SegmentSize) {
    auto& p = Pipelines::instance();
    dm_rs* rs = p.pick();
    if (!rs) return {{}, Error{p.status(), dm_strerror(p.status())}};
    const uint64_t n = objs.size(), total = DataShards + ParShards;
    std::vector<RestoreOutput> out(n);
    std::vector<dm_restore_obj> arr(n);
    std::vector<int> ok(n, 0);
    for (uint64_t o = 0; o < n; o++) {
        const RestoreObject& x = objs[o];
        if (x.frags.size() % total) return {{}, Error{DM_ERR_INVALID, "process: need data + parity fragment entries per segment"}};
        const uint64_t ns = x.frags.size() / total;
        out[o].data.resize(x.size ? x.size : 1);
        out[o].frag_status.resize(ns * total);
        out[o].seg_status.resize(ns);
        dm_restore_obj& a = arr[o];
        a.frags = x.frags.data();
        a.frag_names = x.frag_names.empty() ? nullptr : x.frag_names.data();
        a.seg_names = x.seg_names.empty() ? nullptr : x.seg_names.data();
        a.fid = x.fid.empty() ? nullptr : x.fid.data();
        a.nseg = ns;
        a.size = x.size;
        a.flags = x.flags;
        a.cipher = x.cipher.empty() ? nullptr : x.cipher.data();
        a.cipher_len = x.cipher.size();
        a.out = out[o].data.data();
        a.frag_status = out[o].frag_status.data();
        a.seg_status = out[o].seg_status.data();
    }
    const int rc = dm_restore_batch(rs, arr.data(), n, segment, ok.data());
    if (rc != DM_OK) return {{}, last_error(rc)};
    for (uint64_t o = 0; o < n; o++) {
        out[o].ok = ok[o] != 0;
        if (out[o].ok) out[o].data.resize(objs[o].size);
        else out[o].data.clear();
    }
    return {std::move(out), std::nullopt};
}

// RestoreRange(fragDir, segs, size, off, length, cipher) (go/process/range_hip.go): bytes
// [off, off + length) of the object for the HTTP Range of GET /file/open (node/fileHandler.go:399-545),
// from just the fragments that cover them (dm_retrieve_range; dm_range_plan says which, so a gateway
// fetches only those).  Every fragment read is checked against its name, a lost one is rebuilt from
// any DataShards others and must equal its name; segment names and the fid are not checked (they name
// whole segments).  cipher: "" or the 16 / 24 / 32 bytes the object was processed with (the scheme
// is recalled, not pinned: deoss_amd/csrc/cipher_scheme.hpp); size, off and length count plaintext.
inline std::pair<std::vector<uint8_t>, std::optional<Error>> RestoreRange(const std::string& fragdir,
                                                                           const std::vector<SegmentDataInfo>& segs,
                                                                           uint64_t size, uint64_t off, uint64_t length,
                                                                           const std::string& cipher = "") {
    auto base32 = [](const std::string& path, uint8_t* out) -> bool {
        const std::string n = path.substr(path.rfind('/') == std::string::npos ? 0 : path.rfind('/') + 1);
        auto nib = [](char ch) -> int { return ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1; };
        if (n.size() != 64) return false;
        for (int i = 0; i < 32; i++) {
            const int hi = nib(n[2 * i]), lo = nib(n[2 * i + 1]);
            if (hi < 0 || lo < 0) return false;
            out[i] = (uint8_t)(hi * 16 + lo);
        }
        return true;
    };
    const int total = DataShards + ParShards;
    std::vector<uint8_t> fragn(32 * segs.size() * total), sst(segs.size());
    for (size_t s = 0; s < segs.size(); s++) {
        bool ok = (int)segs[s].FragmentHash.size() == total;
        for (int j = 0; ok && j < total; j++) ok = base32(segs[s].FragmentHash[j], fragn.data() + 32 * (s * total + j));
        if (!ok) return {{}, Error{DM_ERR_INVALID, "process: fragment names must be hex SHA-256"}};
    }
    auto& p = Pipelines::instance();
    dm_rs* rs = p.pick();
    if (!rs) return {{}, Error{p.status(), dm_strerror(p.status())}};
    std::vector<uint8_t> out(length ? length : 1);
    int ok = 0;
    const int rc = dm_retrieve_range(rs, fragdir.c_str(), fragn.data(), segs.size(), size, SegmentSize, off, length,
                                     DM_RESTORE_VERIFY_FRAGMENTS, cipher.empty() ? nullptr : cipher.data(), cipher.size(),
                                     out.data(), nullptr, sst.data(), &ok);
    if (rc != DM_OK) return {{}, last_error(rc)};
    if (!ok) {
        for (uint8_t st : sst)
            if (st == 3) return {{}, Error{DM_ERR_INVALID, "process: restore failed: bad padding after decryption (wrong cipher?)"}};
        return {{}, Error{DM_ERR_INVALID, "process: restore failed: too few verified fragments or a rebuilt fragment mismatch"}};
    }
    out.resize(length);
    return {std::move(out), std::nullopt};
}

// RepairFragments(fragDir, segs, scrub) (go/process/repair_hip.go): what DeOSS's tracker needs when
// a fragment file went missing (node/tracker.go:320-355), without the object and without the
// cipher.  segs is what FullProcessing returned; every fragment file of theirs that is missing from
// fragDir or has the wrong length -- with scrub: or does not equal its name -- is rebuilt from the
// other fragments of its segment (dm_repair_files) and appears under its name only after its
// SHA-256 matched.  first: files rebuilt, also when some segment had too few good fragments left.
inline std::pair<uint64_t, std::optional<Error>> RepairFragments(const std::string& fragdir,
                                                                 const std::vector<SegmentDataInfo>& segs,
                                                                 bool scrub = false) {
    auto base32 = [](const std::string& path, uint8_t* out) -> bool {
        const std::string n = path.substr(path.rfind('/') == std::string::npos ? 0 : path.rfind('/') + 1);
        auto nib = [](char ch) -> int { return ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1; };
        if (n.size() != 64) return false;
        for (int i = 0; i < 32; i++) {
            const int hi = nib(n[2 * i]), lo = nib(n[2 * i + 1]);
            if (hi < 0 || lo < 0) return false;
            out[i] = (uint8_t)(hi * 16 + lo);
        }
        return true;
    };
    const int total = DataShards + ParShards;
    std::vector<uint8_t> fragn(32 * segs.size() * total);
    for (size_t s = 0; s < segs.size(); s++) {
        bool ok = (int)segs[s].FragmentHash.size() == total;
        for (int j = 0; ok && j < total; j++) ok = base32(segs[s].FragmentHash[j], fragn.data() + 32 * (s * total + j));
        if (!ok) return {0, Error{DM_ERR_INVALID, "process: fragment names must be hex SHA-256"}};
    }
    auto& p = Pipelines::instance();
    dm_rs* rs = p.pick();
    if (!rs) return {0, Error{p.status(), dm_strerror(p.status())}};
    int ok = 0;
    uint64_t n = 0;
    const int rc = dm_repair_files(rs, fragdir.c_str(), fragn.data(), segs.size(), SegmentSize, scrub ? DM_REPAIR_SCRUB : 0,
                                   nullptr, nullptr, &n, &ok);
    if (rc != DM_OK) return {n, last_error(rc)};
    if (!ok) return {n, Error{DM_ERR_INVALID, "process: repair failed: too few verified fragments or a fragment mismatch"}};
    return {n, std::nullopt};
}

// FullProcessing while the body arrives (dm_pstream_*): Write the pieces, then Close.
class Writer {
  public:
    static std::pair<std::unique_ptr<Writer>, std::optional<Error>> New(const std::string& savedir) {
        auto& p = Pipelines::instance();
        dm_rs* rs = p.pick();
        if (!rs) return {nullptr, Error{p.status(), dm_strerror(p.status())}};
        std::unique_ptr<Writer> w(new Writer(savedir));
        const int rc = dm_pstream_open(rs, SegmentSize, savedir.c_str(), write_segments() ? DM_FP_SEGMENT_FILES : 0, &w->st_);
        if (rc != DM_OK) return {nullptr, last_error(rc)};
        return {std::move(w), std::nullopt};
    }
    std::optional<Error> Write(const void* p, uint64_t len) {
        if (!st_) return Error{DM_ERR_INVALID, "process: write on a closed Writer"};
        const int rc = dm_pstream_write(st_, p, len);
        if (rc != DM_OK) {
            Error e = last_error(rc);
            Abort();
            return e;
        }
        n_ += len;
        return std::nullopt;
    }
    Result Close() {
        if (!st_) return {{}, "", Error{DM_ERR_INVALID, "process: Writer already closed"}};
        const uint64_t cap = std::max<uint64_t>(1, (n_ + SegmentSize - 1) / SegmentSize);
        std::vector<uint8_t> segd(32 * cap), fragd(32 * cap * (DataShards + ParShards));
        uint8_t fid[32];
        uint64_t nseg = 0;
        dm_pstream* st = st_;
        st_ = nullptr;
        const int rc = dm_pstream_close(st, segd.data(), fragd.data(), cap, &nseg, fid);
        if (rc != DM_OK) return {{}, "", last_error(rc)};
        return {infos(savedir_, segd, fragd, nseg), hex32(fid), std::nullopt};
    }
    void Abort() {
        if (st_) dm_pstream_abort(st_);
        st_ = nullptr;
    }
    ~Writer() { Abort(); }

  private:
    explicit Writer(std::string savedir) : savedir_(std::move(savedir)) {}
    std::string savedir_;
    dm_pstream* st_ = nullptr;
    uint64_t n_ = 0;
};

}  // namespace process
