// GPU test program of the C++ mirror's batch form (include/deoss_process.hpp): runs
// process::FullProcessingCipherBatch over the objects a manifest names and prints every object's
// fid, digests and fragments in hex, for tests/test_cipher_keyed_gpu.py to compare with the CPU
// reference.
//   test_cipher_batch_mirror <manifest> <segment>
// manifest: one line per object, "<file> <cipher in hex, or - for none>".
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

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s manifest segment\n", argv[0]);
        return 2;
    }
    const uint64_t segment = std::strtoull(argv[2], nullptr, 10);
    std::vector<std::vector<char>> bodies;
    std::vector<std::string> ciphers;
    std::ifstream mf(argv[1]);
    std::string line;
    while (std::getline(mf, line)) {
        std::istringstream ls(line);
        std::string path, key;
        if (!(ls >> path >> key)) continue;
        std::ifstream f(path, std::ios::binary);
        if (!f) {
            std::fprintf(stderr, "cannot open %s\n", path.c_str());
            return 2;
        }
        bodies.emplace_back(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
        std::string raw;
        if (key != "-")
            for (size_t i = 0; i + 1 < key.size(); i += 2) raw.push_back((char)std::strtoul(key.substr(i, 2).c_str(), nullptr, 16));
        ciphers.push_back(raw);
    }
    std::vector<process::BatchObject> objs(bodies.size());
    for (size_t o = 0; o < bodies.size(); o++) objs[o] = process::BatchObject{bodies[o].data(), bodies[o].size(), ciphers[o]};
    // a cipher of the wrong length on one object is the library's error, naming the object
    if (objs.size() > 1) {
        std::vector<process::BatchObject> bad = objs;
        bad[1].cipher = "fifteen-bytes-x";
        auto [out, err] = process::FullProcessingCipherBatch(bad, true, segment);
        if (!err || err->code != DM_ERR_INVALID || err->message.find("object 1") == std::string::npos ||
            err->message.find("cipher must be 16, 24 or 32 bytes") == std::string::npos || !out.empty()) {
            std::fprintf(stderr, "15-byte cipher: expected DM_ERR_INVALID naming object 1, got %s\n",
                         err ? err->message.c_str() : "no error");
            return 1;
        }
    }
    auto [out, err] = process::FullProcessingCipherBatch(objs, true, segment);
    if (err) {
        std::fprintf(stderr, "FullProcessingCipherBatch: %d %s\n", err->code, err->message.c_str());
        return 1;
    }
    std::printf("NOBJ %zu\n", out.size());
    for (const auto& o : out)
        std::printf("OBJ %s %s %s %s\n", o.fid.c_str(), hex(o.seg_hashes).c_str(), hex(o.frag_hashes).c_str(), hex(o.frags).c_str());
    std::printf("PASS\n");
    return 0;
}
