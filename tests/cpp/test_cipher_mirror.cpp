// GPU test program of the C++ mirror's cipher path (include/deoss_process.hpp): runs
// process::FullProcessingCipher(file, cipher, savedir, segment) and prints the fid, the segment
// count and every name, for tests/test_cipher_gpu.py to compare with the CPU reference.
//   test_cipher_mirror <file> <cipher> <savedir> <segment>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "deoss_process.hpp"

int main(int argc, char** argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s file cipher savedir segment\n", argv[0]);
        return 2;
    }
    const uint64_t segment = std::strtoull(argv[4], nullptr, 10);
    // a cipher of the wrong length is the library's error, passed through
    {
        auto [info, fid, err] = process::FullProcessingCipher(argv[1], "fifteen-bytes-x", argv[3], segment);
        if (!err || err->code != DM_ERR_INVALID || err->message.find("cipher must be 16, 24 or 32 bytes") == std::string::npos ||
            !info.empty() || !fid.empty()) {
            std::fprintf(stderr, "15-byte cipher: expected DM_ERR_INVALID, got %s\n", err ? err->message.c_str() : "no error");
            return 1;
        }
    }
    auto [info, fid, err] = process::FullProcessingCipher(argv[1], argv[2], argv[3], segment);
    if (err) {
        std::fprintf(stderr, "FullProcessingCipher: %d %s\n", err->code, err->message.c_str());
        return 1;
    }
    std::printf("FID %s\nNSEG %zu\n", fid.c_str(), info.size());
    for (const auto& s : info) {
        std::printf("SEG %s\n", s.SegmentHash.c_str());
        for (const auto& f : s.FragmentHash) std::printf("FRAG %s\n", f.c_str());
    }
    std::printf("PASS\n");
    return 0;
}
