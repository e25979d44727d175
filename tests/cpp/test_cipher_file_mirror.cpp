// GPU test program of the C++ mirror's one-call cipher path (include/deoss_process.hpp): runs
// process::FullProcessing(file, cipher, savedir, segment) -- dm_full_processing_cipher -- and prints
// the fid, the segment count and every name, for tests/test_cipher_file_gpu.py to compare with the
// CPU reference.  The window path (FullProcessingCipher) must still give the same.
//   test_cipher_file_mirror <file> <cipher> <savedir> <segment>
#include <cstdio>
#include <cstdlib>
#include <string>

#include <sys/stat.h>

#include "deoss_process.hpp"

int main(int argc, char** argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s file cipher savedir segment\n", argv[0]);
        return 2;
    }
    const uint64_t segment = std::strtoull(argv[4], nullptr, 10);
    // a cipher of the wrong length is the library's error, passed through, and savedir is not made
    {
        auto [info, fid, err] = process::FullProcessing(argv[1], "fifteen-bytes-x", argv[3], segment);
        struct stat st {};
        if (!err || err->code != DM_ERR_INVALID || err->message.find("cipher must be 16, 24 or 32 bytes") == std::string::npos ||
            !info.empty() || !fid.empty() || ::stat(argv[3], &st) == 0) {
            std::fprintf(stderr, "15-byte cipher: expected DM_ERR_INVALID and no savedir, got %s\n",
                         err ? err->message.c_str() : "no error");
            return 1;
        }
    }
    auto [info, fid, err] = process::FullProcessing(argv[1], argv[2], argv[3], segment);
    if (err) {
        std::fprintf(stderr, "FullProcessing: %d %s\n", err->code, err->message.c_str());
        return 1;
    }
    // the window path stays callable and agrees (its files are the same names: nothing new is written)
    {
        auto [winfo, wfid, werr] = process::FullProcessingCipher(argv[1], argv[2], argv[3], segment);
        if (werr || wfid != fid || winfo.size() != info.size()) {
            std::fprintf(stderr, "FullProcessingCipher disagrees: %s\n", werr ? werr->message.c_str() : wfid.c_str());
            return 1;
        }
        for (size_t s = 0; s < info.size(); s++)
            if (winfo[s].SegmentHash != info[s].SegmentHash || winfo[s].FragmentHash != info[s].FragmentHash) {
                std::fprintf(stderr, "FullProcessingCipher: segment %zu has other names\n", s);
                return 1;
            }
    }
    std::printf("FID %s\nNSEG %zu\n", fid.c_str(), info.size());
    for (const auto& s : info) {
        std::printf("SEG %s\n", s.SegmentHash.c_str());
        for (const auto& f : s.FragmentHash) std::printf("FRAG %s\n", f.c_str());
    }
    std::printf("PASS\n");
    return 0;
}
