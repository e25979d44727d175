// fp_files.hpp -- the files a FullProcessing call writes (pure host code: POSIX only, no HIP).
//
// Shared by dm_full_processing (fullproc_capi.inl), the processing stream (process_stream.inl),
// dm_fragment_lookup and the restore path (its fragment reads and output writes, Go-style error
// texts, FdGuard, env_bytes), and by the host tests (tests/cpp/test_fp_files.cpp, plain and ASan/UBSan, no GPU).
//
// Every output file is written under a temporary name in the save directory while the GPU still
// hashes it, and renamed to <hex SHA-256> once its digest is back (FpOutputs).  Error texts are
// Go's ("open <path>: no such file or directory"): the Go bindings and their tests match on them.
#pragma once

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <future>
#include <string>
#include <utility>
#include <vector>

#include "fp_layout.hpp"

namespace dm_fp {

constexpr int kFpWritersPerSlot = 4;   // background write jobs per parity slot

// Go's error text for an errno: strerror with a lower-case first letter ("no such file or directory").
inline std::string go_errno(int e) {
    std::string m = std::strerror(e);
    if (!m.empty()) m[0] = (char)std::tolower((unsigned char)m[0]);
    return m;
}

struct FdGuard {
    int fd = -1;
    ~FdGuard() {
        if (fd >= 0) ::close(fd);
    }
};

inline uint64_t env_bytes(const char* name, uint64_t dflt) {
    const char* v = std::getenv(name);
    const unsigned long long x = v ? std::strtoull(v, nullptr, 10) : 0;
    return x ? (uint64_t)x : dflt;
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

// os.WriteFile(path, data, os.ModePerm), as the Go shim writes fragments; "" on success.
inline std::string write_whole(const std::string& path, const uint8_t* p, uint64_t len) {
    const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0777);
    if (fd < 0) return "open " + path + ": " + go_errno(errno);
    uint64_t done = 0;
    while (done < len) {
        const ssize_t w = ::write(fd, p + done, len - done);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) {
            const int e = w < 0 ? errno : EIO;
            ::close(fd);
            return "write " + path + ": " + go_errno(e);
        }
        done += (uint64_t)w;
    }
    if (::close(fd) != 0) return "close " + path + ": " + go_errno(errno);
    return "";
}

// os.MkdirAll(dir, 0755)
inline std::string mkdir_all(const std::string& dir) {
    for (size_t i = 1; i <= dir.size(); i++) {
        if (i < dir.size() && dir[i] != '/') continue;
        const std::string p = dir.substr(0, i);
        struct stat st {};
        if (::stat(p.c_str(), &st) == 0) {
            if (!S_ISDIR(st.st_mode)) return "mkdir " + p + ": not a directory";
            continue;
        }
        if (::mkdir(p.c_str(), 0755) != 0 && errno != EEXIST) return "mkdir " + p + ": " + go_errno(errno);
    }
    return "";
}

struct FpFile {          // one file to write: its bytes (memory, or a range of an open file) and temporary name
    const uint8_t* src;
    uint64_t len;
    std::string tmp;
    int in_fd = -1;         // >= 0: the bytes are [in_off, in_off + len) of this file (copied in the kernel)
    uint64_t in_off = 0;
};

// A file range into a new file: copy_file_range (page cache to page cache in the kernel, no user
// copy), or pread / write through a bounce buffer where the kernel cannot.
inline std::string copy_whole(const std::string& path, int in_fd, uint64_t off, uint64_t len) {
    const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0777);
    if (fd < 0) return "open " + path + ": " + go_errno(errno);
    uint64_t done = 0;
    bool kernel = true;
    std::vector<uint8_t> bounce;
    while (done < len) {
        if (kernel) {
            loff_t io = (loff_t)(off + done);
            const ssize_t w = ::copy_file_range(in_fd, &io, fd, nullptr, len - done, 0);
            if (w > 0) {
                done += (uint64_t)w;
                continue;
            }
            if (w < 0 && errno == EINTR) continue;
            if (w < 0 && errno != EXDEV && errno != ENOSYS && errno != EINVAL && errno != EOPNOTSUPP) {
                const int e = errno;
                ::close(fd);
                return "write " + path + ": " + go_errno(e);
            }
            kernel = false;   // 0 (short source) or unsupported: finish through user space
            bounce.resize(8ull << 20);
        }
        const uint64_t n = std::min<uint64_t>(bounce.size(), len - done);
        const ssize_t r = ::pread(in_fd, bounce.data(), n, (off_t)(off + done));
        if (r <= 0) {
            ::close(fd);
            return "read: " + (r < 0 ? go_errno(errno) : std::string("unexpected EOF"));
        }
        for (ssize_t put = 0; put < r;) {
            const ssize_t w = ::write(fd, bounce.data() + put, (size_t)(r - put));
            if (w < 0 && errno == EINTR) continue;
            if (w <= 0) {
                const int e = w < 0 ? errno : EIO;
                ::close(fd);
                return "write " + path + ": " + go_errno(e);
            }
            put += w;
        }
        done += (uint64_t)r;
    }
    if (::close(fd) != 0) return "close " + path + ": " + go_errno(errno);
    return "";
}

// Background writes out of one pinned slot; wait() joins them before the slot is refilled.
struct SlotWrites {
    std::vector<std::future<std::string>> jobs;
    void start(std::vector<FpFile> files, size_t jobs_max = kFpWritersPerSlot) {
        const size_t J = std::min<size_t>(jobs_max, files.size());
        for (size_t j = 0; j < J; j++) {
            std::vector<FpFile> mine;
            for (size_t i = j; i < files.size(); i += J) mine.push_back(files[i]);
            jobs.push_back(std::async(std::launch::async, [mine]() {
                for (const auto& f : mine) {
                    std::string e = f.in_fd >= 0 ? copy_whole(f.tmp, f.in_fd, f.in_off, f.len)
                                                 : write_whole(f.tmp, f.src, f.len);
                    if (!e.empty()) return e;
                }
                return std::string();
            }));
        }
    }
    std::string wait() {   // first error, once every job has finished
        std::string err;
        for (auto& j : jobs) {
            std::string e = j.get();
            if (err.empty()) err = e;
        }
        jobs.clear();
        return err;
    }
    ~SlotWrites() { (void)wait(); }
};

// The restore path's reads: file i of `paths` (len bytes each) to buf + i * len, up to `readers`
// files at a time; the first error ("open P: ...", "read P: ...", "read P: unexpected EOF" for a
// short file) once every reader has finished, "" on success.  (Tested in tests/cpp/test_rs_plan.cpp.)
inline std::string read_files(const std::string* paths, size_t n, uint64_t len, uint8_t* buf, size_t readers) {
    const size_t J = std::min(readers, n);
    std::vector<std::future<std::string>> jobs;
    for (size_t j = 0; j < J; j++)
        jobs.push_back(std::async(std::launch::async, [=]() -> std::string {
            for (size_t i = j; i < n; i += J) {
                const std::string& p = paths[i];
                const int fd = ::open(p.c_str(), O_RDONLY | O_CLOEXEC);
                if (fd < 0) return "open " + p + ": " + go_errno(errno);
                uint64_t done = 0;
                while (done < len) {
                    const ssize_t got = ::pread(fd, buf + i * len + done, len - done, (off_t)done);
                    if (got < 0 && errno == EINTR) continue;
                    if (got <= 0) {
                        const std::string e = got < 0 ? go_errno(errno) : std::string("unexpected EOF");
                        ::close(fd);
                        return "read " + p + ": " + e;
                    }
                    done += (uint64_t)got;
                }
                ::close(fd);
            }
            return std::string();
        }));
    std::string err;
    for (auto& j : jobs) {
        const std::string e = j.get();
        if (err.empty()) err = e;
    }
    return err;
}

// len bytes to [off, off + len) of the open file fd (`path` names it in the error); "" on success.
inline std::string pwrite_all(int fd, const std::string& path, const uint8_t* p, uint64_t len, uint64_t off) {
    uint64_t done = 0;
    while (done < len) {
        const ssize_t w = ::pwrite(fd, p + done, len - done, (off_t)(off + done));
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) return "write " + path + ": " + go_errno(w < 0 ? errno : EIO);
        done += (uint64_t)w;
    }
    return "";
}

inline std::atomic<uint64_t> g_fp_seq{0};   // one counter for every call's temporary names

// The output files of one call: the save directory, the call's temporary names and, per file
// written, the tag of the digest that will name it (fp_layout.hpp).
struct FpOutputs {
    std::string dir, base;
    std::vector<std::pair<std::string, uint64_t>> pend;   // temporary name ("" once renamed), tag

    // savedir without trailing slashes; temporaries are <dir>/<prefix><pid>-<call number>-...
    void open(const char* savedir, const char* prefix) {
        dir = savedir;
        while (dir.size() > 1 && dir.back() == '/') dir.pop_back();
        base = dir + "/" + prefix + std::to_string((long long)::getpid()) + "-" +
               std::to_string((unsigned long long)g_fp_seq++) + "-";
    }
    const std::string& add_frag(uint64_t frag_id) {
        pend.emplace_back(base + "f" + std::to_string(frag_id), frag_tag(frag_id));
        return pend.back().first;
    }
    const std::string& add_seg(uint64_t gs) {
        pend.emplace_back(base + "s" + std::to_string(gs), seg_tag(gs));
        return pend.back().first;
    }

    // The data-fragment files (and, if seg_file, the segment file) of the object's segment gs, whose
    // bytes are at `src` or, when src is null, at [in_off, in_off + seg) of in_fd; appended to files.
    void data_files(const FpLayout& L, uint64_t gs, const uint8_t* src, int in_fd, uint64_t in_off, bool seg_file,
                    std::vector<FpFile>& files) {
        auto add = [&](uint64_t off, uint64_t len, const std::string& tmp) {
            if (src) files.push_back({src + off, len, tmp});
            else files.push_back({nullptr, len, tmp, in_fd, in_off + off});
        };
        for (int j = 0; j < L.k; j++) add((uint64_t)j * L.frag, L.frag, add_frag(L.frag_id(gs, j)));
        if (seg_file) add(0, L.seg, add_seg(gs));
    }
    // The parity-fragment files of segments [gs0, gs0 + nt), whose parity sets lie back to back at buf.
    std::vector<FpFile> parity_files(const FpLayout& L, uint64_t gs0, uint64_t nt, const uint8_t* buf) {
        std::vector<FpFile> files;
        for (uint64_t u = 0; u < nt; u++)
            for (int i = 0; i < L.m; i++)
                files.push_back({buf + u * L.pbytes + (uint64_t)i * L.frag, L.frag, add_frag(L.frag_id(gs0 + u, L.k + i))});
        return files;
    }

    // Every temporary to dir/<hex digest> ("" on success, else "rename A B: <errno text>").
    std::string rename_all(const uint8_t* segd, const uint8_t* fragd) {
        for (auto& p : pend) {
            if (p.first.empty()) continue;
            const std::string to = dir + "/" + hex32(tag_digest(segd, fragd, p.second));
            if (::rename(p.first.c_str(), to.c_str()) != 0)
                return "rename " + p.first + " " + to + ": " + go_errno(errno);
            p.first.clear();
        }
        return "";
    }
    void unlink_pending() {   // no temporary survives a failed call
        for (const auto& p : pend)
            if (!p.first.empty()) ::unlink(p.first.c_str());
    }
};

}  // namespace dm_fp
