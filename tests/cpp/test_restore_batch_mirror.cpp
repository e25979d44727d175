// GPU test program of the C++ mirror's batched restore (include/deoss_process.hpp): runs
// process::RestoreBatch over the objects a manifest names and prints every object's verdict, bytes
// and segment statuses in hex, for tests/test_restore_batch_gpu.py to compare with the reference.
//   test_restore_batch_mirror <manifest> <segment>
// manifest: one line per object, "<fragments file> <names file> <presence> <nseg> <size> <flags>
// <cipher in hex, or - for none>": the fragments file holds the fragments that are present, in
// order; presence is one '0' / '1' per fragment; the names file holds the fragment names, the
// segment names and the fid.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "deoss_process.hpp"

static std::string hex(const std::vector<uint8_t>& v) {
    static const char* x = "0123456789abcdef";
    std::string s;
    s.reserve(2 * v.size());
    for (uint8_t b : v) {
        s.push_back(x[b >> 4]);
        s.push_back(x[b & 15]);
    }
    return s;
}

static bool slurp(const std::string& path, std::vector<char>& out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path.c_str());
        return false;
    }
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s manifest segment\n", argv[0]);
        return 2;
    }
    const uint64_t segment = std::strtoull(argv[2], nullptr, 10);
    const uint64_t total = process::DataShards + process::ParShards, frag = segment / process::DataShards;
    std::vector<std::vector<char>> bodies;   // the fragments stay where RestoreObject::frags points
    std::vector<process::RestoreObject> objs;
    std::ifstream mf(argv[1]);
    std::string line;
    while (std::getline(mf, line)) {
        std::istringstream ls(line);
        std::string fpath, npath, present, key;
        uint64_t nseg = 0, size = 0;
        int flags = 0;
        if (!(ls >> fpath >> npath >> present >> nseg >> size >> flags >> key)) continue;
        std::vector<char> names;
        bodies.emplace_back();
        if (!slurp(fpath, bodies.back()) || !slurp(npath, names)) return 2;
        if (present.size() != nseg * total || names.size() != 32 * (nseg * total + nseg + 1)) {
            std::fprintf(stderr, "manifest line does not match its files: %s\n", line.c_str());
            return 2;
        }
        process::RestoreObject x;
        uint64_t at = 0;
        for (char c : present) x.frags.push_back(c == '1' ? bodies.back().data() + (at++) * frag : nullptr);
        if (at * frag != bodies.back().size()) {
            std::fprintf(stderr, "%s: %zu bytes for %llu fragments\n", fpath.c_str(), bodies.back().size(), (unsigned long long)at);
            return 2;
        }
        const uint8_t* nm = reinterpret_cast<const uint8_t*>(names.data());
        x.frag_names.assign(nm, nm + 32 * nseg * total);
        x.seg_names.assign(nm + 32 * nseg * total, nm + 32 * (nseg * total + nseg));
        x.fid.assign(nm + 32 * (nseg * total + nseg), nm + names.size());
        x.size = size;
        x.flags = flags;
        if (key != "-")
            for (size_t i = 0; i + 1 < key.size(); i += 2) x.cipher.push_back((char)std::strtoul(key.substr(i, 2).c_str(), nullptr, 16));
        objs.push_back(std::move(x));
    }
    // the pointers above were taken while `bodies` grew: take them again now that it is final
    for (size_t o = 0; o < objs.size(); o++) {
        uint64_t at = 0;
        for (auto& f : objs[o].frags)
            if (f) f = bodies[o].data() + (at++) * frag;
    }
    // a cipher of the wrong length on one object is the library's error, naming the object
    if (objs.size() > 1) {
        std::vector<process::RestoreObject> bad = objs;
        bad[1].cipher = "fifteen-bytes-x";
        auto [out, err] = process::RestoreBatch(bad, segment);
        if (!err || err->code != DM_ERR_INVALID || err->message.find("object 1") == std::string::npos ||
            err->message.find("cipher must be 16, 24 or 32 bytes") == std::string::npos || !out.empty()) {
            std::fprintf(stderr, "15-byte cipher: expected DM_ERR_INVALID naming object 1, got %s\n",
                         err ? err->message.c_str() : "no error");
            return 1;
        }
    }
    auto [out, err] = process::RestoreBatch(objs, segment);
    if (err) {
        std::fprintf(stderr, "RestoreBatch: %d %s\n", err->code, err->message.c_str());
        return 1;
    }
    std::printf("NOBJ %zu\n", out.size());
    for (const auto& o : out)
        std::printf("OBJ %d %s %s\n", o.ok ? 1 : 0, o.ok ? hex(o.data).c_str() : "-", hex(o.seg_status).c_str());
    std::printf("PASS\n");
    return 0;
}
