// Host test of the FullProcessing output files (deoss_amd/csrc/fp_files.hpp): no GPU, built plain
// and with ASan/UBSan by tests/test_fp_host.py.  argv[1]: an empty scratch directory.
//
//  1. hex32 against a fixed vector; go_errno's lower-case first letter;
//  2. mkdir_all on a nested path, and "mkdir <p>: not a directory" when a middle component is a file;
//  3. write_whole and copy_whole of 0, 1 and 3 MiB + 1 bytes (copy_whole from a non-zero offset);
//     copy_whole from a range past EOF fails with "unexpected EOF";
//  4. SlotWrites returns the first error after every job has ended;
//  5. FpOutputs: rename_all leaves exactly the hex names (two files with equal digests end as one),
//     a rename failure (the target is a directory) followed by unlink_pending leaves no .dm-
//     temporary behind.
#include <dirent.h>

#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../deoss_amd/csrc/fp_files.hpp"

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

static std::vector<uint8_t> pattern(uint64_t n, uint64_t seed) {
    std::vector<uint8_t> v(n);
    uint64_t x = seed * 0x9e3779b97f4a7c15ull + 1;
    for (uint64_t i = 0; i < n; i++) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        v[i] = (uint8_t)(x >> 56);
    }
    return v;
}

static bool read_file(const std::string& p, std::vector<uint8_t>& out) {
    FILE* f = std::fopen(p.c_str(), "rb");
    if (!f) return false;
    out.clear();
    uint8_t buf[1 << 16];
    for (size_t r; (r = std::fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + r);
    std::fclose(f);
    return true;
}

static std::set<std::string> ls(const std::string& dir) {
    std::set<std::string> names;
    DIR* d = ::opendir(dir.c_str());
    if (!d) return names;
    while (struct dirent* e = ::readdir(d))
        if (std::strcmp(e->d_name, ".") != 0 && std::strcmp(e->d_name, "..") != 0) names.insert(e->d_name);
    ::closedir(d);
    return names;
}

static void check_text() {
    uint8_t d[32];
    for (int i = 0; i < 32; i++) d[i] = (uint8_t)(i * 9 + (i == 31 ? 0xe0 : 0));
    CHECK(hex32(d) == "0009121b242d363f48515a636c757e879099a2abb4bdc6cfd8e1eaf3fc050ef7", "hex32: %s", hex32(d).c_str());
    CHECK(go_errno(ENOENT) == "no such file or directory", "go_errno: %s", go_errno(ENOENT).c_str());
    CHECK(go_errno(EISDIR) == "is a directory", "go_errno: %s", go_errno(EISDIR).c_str());
}

static void check_mkdir(const std::string& root) {
    const std::string deep = root + "/a/b/c";
    CHECK(mkdir_all(deep).empty(), "mkdir_all nested: %s", mkdir_all(deep).c_str());
    struct stat st {};
    CHECK(::stat(deep.c_str(), &st) == 0 && S_ISDIR(st.st_mode), "nested directory missing");
    CHECK(mkdir_all(deep).empty(), "mkdir_all of an existing path");
    const std::string file = root + "/a/plain";
    CHECK(write_whole(file, nullptr, 0).empty(), "write_whole of an empty file");
    const std::string e = mkdir_all(file + "/x/y");
    CHECK(e == "mkdir " + file + ": not a directory", "mkdir through a file: '%s'", e.c_str());
}

static void check_writes(const std::string& root) {
    const uint64_t sizes[] = {0, 1, (3ull << 20) + 1};
    const uint64_t off = 12345;
    for (uint64_t n : sizes) {
        const std::vector<uint8_t> src = pattern(off + n + 77, n + 1);
        const std::string in = root + "/in" + std::to_string(n), w = root + "/w" + std::to_string(n),
                          c = root + "/c" + std::to_string(n);
        CHECK(write_whole(in, src.data(), src.size()).empty(), "write_whole source of %llu", (unsigned long long)n);
        CHECK(write_whole(w, src.data() + off, n).empty(), "write_whole of %llu", (unsigned long long)n);
        std::vector<uint8_t> got;
        CHECK(read_file(w, got) && got == std::vector<uint8_t>(src.begin() + (ptrdiff_t)off, src.begin() + (ptrdiff_t)(off + n)),
              "write_whole content of %llu", (unsigned long long)n);
        FdGuard fd;
        fd.fd = ::open(in.c_str(), O_RDONLY | O_CLOEXEC);
        CHECK(fd.fd >= 0, "open %s", in.c_str());
        const std::string e = copy_whole(c, fd.fd, off, n);
        CHECK(e.empty(), "copy_whole of %llu: %s", (unsigned long long)n, e.c_str());
        CHECK(read_file(c, got) && got == std::vector<uint8_t>(src.begin() + (ptrdiff_t)off, src.begin() + (ptrdiff_t)(off + n)),
              "copy_whole content of %llu", (unsigned long long)n);
        // a range that runs past the end of the source
        const std::string past = copy_whole(root + "/past" + std::to_string(n), fd.fd, off, n + 78);
        CHECK(past == "read: unexpected EOF", "copy_whole past EOF: '%s'", past.c_str());
    }
    // write_whole overwrites (O_TRUNC), and reports Go's text for a missing directory
    const std::vector<uint8_t> a = pattern(100, 1), b = pattern(10, 2);
    std::vector<uint8_t> got;
    CHECK(write_whole(root + "/over", a.data(), a.size()).empty() && write_whole(root + "/over", b.data(), b.size()).empty() &&
              read_file(root + "/over", got) && got == b, "write_whole does not truncate");
    const std::string e = write_whole(root + "/missing/f", a.data(), a.size());
    CHECK(e == "open " + root + "/missing/f: no such file or directory", "write_whole error text: '%s'", e.c_str());
}

static void check_slot_writes(const std::string& root) {
    const std::vector<uint8_t> a = pattern(5000, 3);
    std::vector<FpFile> files;
    for (int i = 0; i < 9; i++) {
        // files 2 and 3 cannot be created; job j writes files j, j + 4, ...: jobs 2 and 3 fail at
        // their first file, jobs 0 and 1 run to their end, and job 2's error is the one reported
        const std::string dir = (i == 2 || i == 3) ? root + "/nodir" + std::to_string(i) : root;
        files.push_back({a.data() + i, 1000, dir + "/sw" + std::to_string(i)});
    }
    SlotWrites w;
    w.start(files);
    CHECK(w.jobs.size() == (size_t)kFpWritersPerSlot, "%zu jobs", w.jobs.size());
    const std::string e = w.wait();
    CHECK(e == "open " + root + "/nodir2/sw2: no such file or directory", "SlotWrites error: '%s'", e.c_str());
    CHECK(w.jobs.empty() && w.wait().empty(), "wait() leaves jobs behind");
    for (int i : {0, 1, 4, 5, 8}) {   // every other job ran to its end
        std::vector<uint8_t> got;
        CHECK(read_file(root + "/sw" + std::to_string(i), got) &&
                  got == std::vector<uint8_t>(a.begin() + i, a.begin() + i + 1000), "file %d of the good jobs", i);
    }
    // a file range as the source, and fewer files than jobs
    FdGuard fd;
    fd.fd = ::open((root + "/sw0").c_str(), O_RDONLY | O_CLOEXEC);
    SlotWrites c;
    c.start({{nullptr, 900, root + "/swc", fd.fd, 100}}, 8);
    CHECK(c.jobs.size() == 1 && c.wait().empty(), "SlotWrites from a file range");
    std::vector<uint8_t> got;
    CHECK(read_file(root + "/swc", got) && got == std::vector<uint8_t>(a.begin() + 100, a.begin() + 1000), "range content");
}

static void digest_of(uint8_t* d, uint64_t v) {
    for (int b = 0; b < 32; b++) d[b] = (uint8_t)(v * 37 + (uint64_t)b);
}

static void check_outputs(const std::string& root) {
    const FpLayout L(2, 1, 64);   // 2 data + 1 parity fragments of 32 bytes
    const uint64_t nseg = 2;
    const std::vector<uint8_t> data = pattern(nseg * L.seg, 5), par = pattern(nseg * L.pbytes, 6);
    std::vector<uint8_t> segd(32 * nseg), fragd(32 * nseg * L.total);
    for (uint64_t gs = 0; gs < nseg; gs++) {
        digest_of(segd.data() + 32 * gs, 100 + gs);
        for (int j = 0; j < L.total; j++) digest_of(fragd.data() + 32 * L.frag_id(gs, j), L.frag_id(gs, j));
    }
    // fragment (1, 0) has the digest of fragment (0, 0): two files, one name
    std::memcpy(fragd.data() + 32 * L.frag_id(1, 0), fragd.data() + 32 * L.frag_id(0, 0), 32);

    {   // success
        FpOutputs out;
        out.open((root + "/save///").c_str(), ".dm-fp-");
        CHECK(out.dir == root + "/save", "trailing slashes: %s", out.dir.c_str());
        CHECK(out.base.compare(0, out.dir.size() + 8, out.dir + "/.dm-fp-") == 0 && out.base.back() == '-', "base %s",
              out.base.c_str());
        CHECK(mkdir_all(out.dir).empty(), "mkdir save");
        std::vector<FpFile> files;
        for (uint64_t gs = 0; gs < nseg; gs++) out.data_files(L, gs, data.data() + gs * L.seg, -1, 0, true, files);
        CHECK(files.size() == nseg * 3 && out.pend.size() == nseg * 3, "%zu data files", files.size());
        CHECK(files[0].tmp == out.base + "f0" && files[1].tmp == out.base + "f1" && files[2].tmp == out.base + "s0" &&
                  files[3].tmp == out.base + "f3" && files[5].tmp == out.base + "s1", "temporary names");
        CHECK(files[1].src == data.data() + L.frag && files[1].len == L.frag && files[2].src == data.data() &&
                  files[2].len == L.seg && files[4].src == data.data() + L.seg + L.frag, "data file sources");
        CHECK(out.pend[2].second == seg_tag(0) && out.pend[4].second == frag_tag(4), "tags");
        std::vector<FpFile> pf = out.parity_files(L, 0, nseg, par.data());
        CHECK(pf.size() == nseg && pf[0].tmp == out.base + "f2" && pf[1].tmp == out.base + "f5" &&
                  pf[1].src == par.data() + L.pbytes && pf[1].len == L.frag, "parity files");
        files.insert(files.end(), pf.begin(), pf.end());
        SlotWrites w;
        w.start(files);
        CHECK(w.wait().empty(), "writing the temporaries");
        CHECK(ls(out.dir).size() == 8, "%zu temporaries", ls(out.dir).size());
        const std::string e = out.rename_all(segd.data(), fragd.data());
        CHECK(e.empty(), "rename_all: %s", e.c_str());
        std::set<std::string> want;
        for (uint64_t gs = 0; gs < nseg; gs++) {
            want.insert(hex32(segd.data() + 32 * gs));
            for (int j = 0; j < L.total; j++) want.insert(hex32(fragd.data() + 32 * L.frag_id(gs, j)));
        }
        CHECK(want.size() == 7 && ls(out.dir) == want, "save directory holds %zu names, want %zu", ls(out.dir).size(),
              want.size());
        std::vector<uint8_t> got;   // the later of the two equal names won, as rename(2) does
        CHECK(read_file(out.dir + "/" + hex32(fragd.data()), got) &&
                  got == std::vector<uint8_t>(data.begin() + (ptrdiff_t)L.seg, data.begin() + (ptrdiff_t)(L.seg + L.frag)),
              "content under the shared name");
        CHECK(read_file(out.dir + "/" + hex32(segd.data() + 32), got) &&
                  got == std::vector<uint8_t>(data.begin() + (ptrdiff_t)L.seg, data.end()), "segment file content");
        out.unlink_pending();   // nothing left to remove, nothing renamed is touched
        CHECK(ls(out.dir) == want, "unlink_pending after success removed a file");
    }
    {   // a file range as the source (the open input file)
        FpOutputs out;
        out.open((root + "/save2").c_str(), ".dm-ps-");
        std::vector<FpFile> files;
        out.data_files(L, 7, nullptr, 5, 7 * L.seg, false, files);
        CHECK(files.size() == 2 && files[1].src == nullptr && files[1].in_fd == 5 && files[1].in_off == 7 * L.seg + L.frag &&
                  files[1].tmp == out.base + "f22" && out.pend[1].second == frag_tag(22), "file-range data files");
        CHECK(out.base.find("/.dm-ps-") != std::string::npos, "prefix");
    }
    {   // failure: the name of fragment (0, 1) is taken by a directory
        FpOutputs out;
        out.open((root + "/fail").c_str(), ".dm-fp-");
        CHECK(mkdir_all(out.dir).empty(), "mkdir fail");
        const std::string taken = out.dir + "/" + hex32(fragd.data() + 32 * L.frag_id(0, 1));
        CHECK(mkdir_all(taken + "/full").empty(), "mkdir target");
        std::vector<FpFile> files;
        for (uint64_t gs = 0; gs < nseg; gs++) out.data_files(L, gs, data.data() + gs * L.seg, -1, 0, false, files);
        SlotWrites w;
        w.start(files);
        CHECK(w.wait().empty(), "writing the temporaries");
        const std::string e = out.rename_all(segd.data(), fragd.data());
        const std::string head = "rename " + out.base + "f1 " + taken + ": ";
        CHECK(e.compare(0, head.size(), head) == 0 && e.size() > head.size(), "rename error: '%s'", e.c_str());
        CHECK(e == head + go_errno(EISDIR) || e == head + go_errno(ENOTEMPTY) || e == head + go_errno(EEXIST),
              "rename errno text: '%s'", e.c_str());
        out.unlink_pending();
        for (const std::string& n : ls(out.dir)) CHECK(n.compare(0, 4, ".dm-") != 0, "temporary left behind: %s", n.c_str());
        CHECK(ls(out.dir).size() == 2, "the first rename and the directory stay: %zu entries", ls(out.dir).size());
    }
    CHECK(g_fp_seq.load() >= 3, "call counter");
}

static void check_env() {
    ::setenv("DM_FP_TEST_BYTES", "4096", 1);
    CHECK(env_bytes("DM_FP_TEST_BYTES", 7) == 4096, "env_bytes set");
    ::setenv("DM_FP_TEST_BYTES", "0", 1);
    CHECK(env_bytes("DM_FP_TEST_BYTES", 7) == 7, "env_bytes 0 means default");
    ::unsetenv("DM_FP_TEST_BYTES");
    CHECK(env_bytes("DM_FP_TEST_BYTES", 7) == 7, "env_bytes unset");
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <empty scratch directory>\n", argv[0]);
        return 2;
    }
    const std::string root = argv[1];
    check_text();
    check_env();
    check_mkdir(root);
    check_writes(root);
    check_slot_writes(root);
    check_outputs(root);
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("fp files OK\n");
    return 0;
}
