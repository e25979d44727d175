// deoss_reedsolomon.hpp -- C++ host mirror of the Go reedsolomon shim (go/reedsolomon): the subset
// of github.com/klauspost/reedsolomon v1.12.4's Encoder that cess-go-sdk calls (New, Split, Encode,
// Verify, Reconstruct), over the C ABI (include/deoss_merkle.h: dm_rs_create_wide, dm_rs_encode,
// dm_rs_verify, dm_rs_reconstruct).  klauspost's whole range, dataShards + parityShards <= 256, and
// its error texts; a missing shard is an empty vector.  Every byte is coded on the GPU: within 8 + 8
// by the fragment coder FullProcessing uses, beyond it by the wide kernel.  Only the default matrix;
// an Encoder without parity shards is ErrNotSupported.  Header-only; link -ldeoss_merkle.
#pragma once

#include <cstdint>
#include <memory>
#include <optional>
#include <string>
#include <utility>
#include <vector>

#include "deoss_merkle.h"

namespace reedsolomon {

struct Error {
    int code;
    std::string message;
};

inline Error ErrInvShardNum() {
    return {DM_ERR_INVALID, "cannot create Encoder with less than one data shard or less than zero parity shards"};
}
inline Error ErrMaxShardNum() { return {DM_ERR_INVALID, "cannot create Encoder with more than 256 data+parity shards"}; }
inline Error ErrTooFewShards() { return {DM_ERR_INVALID, "too few shards given"}; }
inline Error ErrShortData() { return {DM_ERR_EMPTY, "not enough data to fill the number of requested shards"}; }
inline Error ErrShardSize() { return {DM_ERR_INVALID, "shard sizes do not match"}; }
inline Error ErrShardNoData() { return {DM_ERR_INVALID, "no shard data"}; }
inline Error ErrNotSupported() { return {DM_ERR_INVALID, "operation not supported"}; }

using Shards = std::vector<std::vector<uint8_t>>;

class Encoder {
  public:
    // reedsolomon.New(dataShards, parityShards) on ctx's first GPU (ctx outlives the Encoder).
    static std::pair<std::unique_ptr<Encoder>, std::optional<Error>> New(dm_ctx* ctx, int dataShards, int parityShards) {
        if (dataShards <= 0 || parityShards < 0) return {nullptr, ErrInvShardNum()};
        if (dataShards + parityShards > 256) return {nullptr, ErrMaxShardNum()};
        if (parityShards == 0) return {nullptr, ErrNotSupported()};
        dm_rs* h = nullptr;
        const int rc = dm_rs_create_wide(ctx, dataShards, parityShards, &h);
        if (rc != DM_OK) return {nullptr, last(ctx, rc)};
        return {std::unique_ptr<Encoder>(new Encoder(ctx, h, dataShards, parityShards)), std::nullopt};
    }
    ~Encoder() { dm_rs_destroy(h_); }
    Encoder(const Encoder&) = delete;
    Encoder& operator=(const Encoder&) = delete;

    int DataShards() const { return data_; }
    int ParityShards() const { return parity_; }

    // Equal data shards (the last zero-padded) plus zeroed parity shards.
    std::pair<Shards, std::optional<Error>> Split(const std::vector<uint8_t>& data) const {
        if (data.empty()) return {{}, ErrShortData()};
        const size_t per = (data.size() + (size_t)data_ - 1) / (size_t)data_;
        Shards out((size_t)(data_ + parity_), std::vector<uint8_t>(per, 0));
        for (size_t i = 0; i < data.size(); i++) out[i / per][i % per] = data[i];
        return {std::move(out), std::nullopt};
    }

    // Fills shards[data:] (allocated by the caller, as klauspost requires) with parity.
    std::optional<Error> Encode(Shards& shards) const {
        size_t size = 0;
        if (auto e = check(shards, false, &size)) return e;
        for (const auto& s : shards)
            if (s.size() != size) return ErrShardSize();
        std::vector<const void*> dp((size_t)data_);
        std::vector<void*> pp((size_t)parity_);
        for (int j = 0; j < data_; j++) dp[(size_t)j] = shards[(size_t)j].data();
        for (int i = 0; i < parity_; i++) pp[(size_t)i] = shards[(size_t)(data_ + i)].data();
        const int rc = dm_rs_encode(h_, dp.data(), pp.data(), size);
        if (rc != DM_OK) return last(ctx_, rc);
        return std::nullopt;
    }

    std::pair<bool, std::optional<Error>> Verify(const Shards& shards) const {
        size_t size = 0;
        if (auto e = check(shards, true, &size)) return {false, e};
        std::vector<const void*> p(shards.size());
        for (size_t i = 0; i < shards.size(); i++) p[i] = shards[i].data();
        int ok = 0;
        const int rc = dm_rs_verify(h_, p.data(), size, &ok);
        if (rc != DM_OK) return {false, last(ctx_, rc)};
        return {ok != 0, std::nullopt};
    }

    // Rebuilds every missing (empty) shard; it allocates them like klauspost.
    std::optional<Error> Reconstruct(Shards& shards) const {
        size_t size = 0;
        if (auto e = check(shards, false, &size)) return e;
        std::vector<uint8_t> present(shards.size());
        size_t have = 0;
        for (size_t i = 0; i < shards.size(); i++) have += present[i] = !shards[i].empty();
        if (have == shards.size()) return std::nullopt;
        if (have < (size_t)data_) return ErrTooFewShards();
        std::vector<void*> p(shards.size());
        for (size_t i = 0; i < shards.size(); i++) {
            if (!present[i]) shards[i].assign(size, 0);
            p[i] = shards[i].data();
        }
        const int rc = dm_rs_reconstruct(h_, p.data(), present.data(), size);
        if (rc != DM_OK) return last(ctx_, rc);
        return std::nullopt;
    }

  private:
    Encoder(dm_ctx* ctx, dm_rs* h, int data, int parity) : ctx_(ctx), h_(h), data_(data), parity_(parity) {}

    static Error last(dm_ctx* ctx, int rc) {   // dm_last_error is the calling thread's message
        const std::string m = dm_last_error(ctx);
        return {rc, m.empty() ? std::string(dm_strerror(rc)) : m};
    }

    std::optional<Error> check(const Shards& shards, bool needAll, size_t* size) const {
        if (shards.size() != (size_t)(data_ + parity_)) return ErrTooFewShards();
        *size = 0;
        for (const auto& s : shards) {
            if (s.empty()) {
                if (needAll) return ErrShardNoData();
                continue;
            }
            if (*size == 0) *size = s.size();
            else if (s.size() != *size) return ErrShardSize();
        }
        if (*size == 0) return ErrShardNoData();
        return std::nullopt;
    }

    dm_ctx* ctx_;
    dm_rs* h_;
    int data_, parity_;
};

}  // namespace reedsolomon
