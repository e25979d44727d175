// cipher_capi.inl -- AES-CBC on the GPU (dm_aes_cbc_*_device_async; include/deoss_merkle.h) and the
// launch helpers dm_process_cipher_buffer / dm_restore_cipher_buffer and the ranged restore
// (range_capi.inl: windows of chains) use.  Part of merkle_capi.hip
// (after rs_capi.inl: the decrypt kernel shares rs_grid and rs_store).
//
// The cipher branch of cess-go-sdk process.FullProcessing / Retrievefile (cipher != ""): the scheme
// is recalled, not pinned (cipher_scheme.hpp); the AES-CBC core is FIPS-197 /
// SP 800-38A.  The key schedule runs on the host per call.  With one key per launch the round keys
// are kernel arguments and never sit in a device buffer; the keyed launch (a key per chain:
// launch_aes_encrypt_keyed) is the one place they do, in the lane's d.aes_keys, which is zeroed in
// stream order right after the kernel and on every error path after the upload.
#include "aes_kernels.hpp"
#include "aes_keyed_plan.hpp"
#include "cipher_scheme.hpp"

namespace {

// A cipher string as the kernels take it: both key schedules and the IV.
struct CipherKey {
    dm_aes::KeySchedule ks;
    uint32_t iv[4];
};

void cipher_set_iv(CipherKey& k, const uint8_t iv[16]) { std::memcpy(k.iv, iv, 16); }

// The scheme's key: the cipher's bytes, IV = its first 16.
int cipher_key(dm_ctx* c, const void* cipher, uint64_t cipher_len, CipherKey& k) {
    if (!cipher || !dm_aes::expand_key(static_cast<const uint8_t*>(cipher), cipher_len, k.ks))
        return fail(c, DM_ERR_INVALID, "%s", dm_cipher::kKeyLenError);
    uint8_t iv[16];
    dm_cipher::iv_of(static_cast<const uint8_t*>(cipher), iv);
    cipher_set_iv(k, iv);
    return DM_OK;
}

template <class F>
void aes_for_rounds(int nr, F&& f) {
    switch (nr) {
        case 10: f(std::integral_constant<int, 10>()); break;
        case 12: f(std::integral_constant<int, 12>()); break;
        default: f(std::integral_constant<int, 14>()); break;
    }
}

// nseg chains in place: `plain` bytes at dev + t * stride become plain + 16 bytes of ciphertext.
hipError_t launch_aes_encrypt(hipStream_t s, const CipherKey& k, uint8_t* dev, uint64_t stride, uint64_t plain,
                              uint64_t nseg) {
    dm::AesEncArgs a{};
    std::memcpy(a.rk.w, k.ks.enc, sizeof a.rk.w);
    std::memcpy(a.iv, k.iv, 16);
    a.dev = dev;
    a.stride = stride;
    a.nblk = plain / 16;
    a.nseg = nseg;
    const dim3 grid((uint32_t)ceil_div(nseg * dm::kAesLanesPerChain, dm::kAesEncThreads)), block(dm::kAesEncThreads);
    aes_for_rounds(k.ks.rounds, [&](auto NR) {
        hipLaunchKernelGGL(dm::aes_cbc_encrypt_kernel<decltype(NR)::value>, grid, block, 0, s, a);
    });
    return hipGetLastError();
}

// Blocks [blk_lo, blk_hi) of the same nseg chains (blk_lo < blk_hi <= plain / 16); the launch that
// ends the data appends the padding block.
hipError_t launch_aes_encrypt_range(hipStream_t s, const CipherKey& k, uint8_t* dev, uint64_t stride, uint64_t plain,
                                    uint64_t nseg, uint64_t blk_lo, uint64_t blk_hi) {
    dm::AesEncRangeArgs a{};
    std::memcpy(a.e.rk.w, k.ks.enc, sizeof a.e.rk.w);
    std::memcpy(a.e.iv, k.iv, 16);
    a.e.dev = dev;
    a.e.stride = stride;
    a.e.nblk = plain / 16;
    a.e.nseg = nseg;
    a.blk_lo = blk_lo;
    a.blk_hi = blk_hi;
    const dim3 grid((uint32_t)ceil_div(nseg * dm::kAesLanesPerChain, dm::kAesEncThreads)), block(dm::kAesEncThreads);
    aes_for_rounds(k.ks.rounds, [&](auto NR) {
        hipLaunchKernelGGL(dm::aes_cbc_encrypt_range_kernel<decltype(NR)::value>, grid, block, 0, s, a);
    });
    return hipGetLastError();
}

// nseg x cipher_bytes of ciphertext -> nseg x (cipher_bytes - 16) of plaintext at out + t * out_stride,
// pad_ok[t] = the padding block was sixteen 0x10 bytes.
hipError_t launch_aes_decrypt(Dev& d, hipStream_t s, const CipherKey& k, const uint8_t* in, uint64_t in_stride,
                              uint64_t cipher_bytes, uint64_t nseg, uint8_t* out, uint64_t out_stride, uint8_t* pad_ok) {
    dm::AesDecArgs a{};
    std::memcpy(a.rk.w, k.ks.dec, sizeof a.rk.w);
    std::memcpy(a.iv, k.iv, 16);
    a.in = in;
    a.in_stride = in_stride;
    a.nblk = cipher_bytes / 16;
    a.nseg = nseg;
    a.out = out;
    a.out_stride = out_stride;
    a.pad_ok = pad_ok;
    const dim3 grid = rs_grid(d, a.nblk, nseg), block(dm::kAesDecThreads);
    static_assert(dm::kAesDecThreads == dm::kRsThreads, "rs_grid sizes x for kRsThreads lanes");
    aes_for_rounds(k.ks.rounds, [&](auto NR) {
        hipLaunchKernelGGL(dm::aes_cbc_decrypt_kernel<decltype(NR)::value>, grid, block, 0, s, a);
    });
    return hipGetLastError();
}

// Windows of chains (aes_cbc_decrypt_window_kernel): the descriptors are uploaded through the lane's
// bounce buffer to d.aes_win, ONE launch decrypts them all.  pad_ok: [win.size()] on the device.
int launch_aes_decrypt_windows(dm_ctx* c, Dev& d, hipStream_t s, const CipherKey& k, const std::vector<dm::AesWindow>& win,
                               uint8_t* pad_ok) {
    if (win.empty()) return DM_OK;
    uint64_t longest = 0;
    for (const dm::AesWindow& w : win) longest = std::max(longest, w.nblk);
    const uint64_t bytes = win.size() * sizeof(dm::AesWindow);
    RC_TRY(tables_begin(c, d, bytes + 1024));
    RC_TRY(upload(c, d, s, d.aes_win, win.data(), bytes));
    dm::AesWinArgs a{};
    std::memcpy(a.rk.w, k.ks.dec, sizeof a.rk.w);
    std::memcpy(a.iv, k.iv, 16);
    a.win = static_cast<const dm::AesWindow*>(d.aes_win.p);
    a.nwin = win.size();
    a.pad_ok = pad_ok;
    const dim3 grid = rs_grid(d, longest, a.nwin), block(dm::kAesDecThreads);
    aes_for_rounds(k.ks.rounds, [&](auto NR) {
        hipLaunchKernelGGL(dm::aes_cbc_decrypt_window_kernel<decltype(NR)::value>, grid, block, 0, s, a);
    });
    HIP_TRY(hipGetLastError());
    return DM_OK;
}

// A chain of a keyed launch: `plain` bytes at dev, encrypted in place under keys[key].
struct KeyedChain {
    uint8_t* dev;
    uint32_t key;
};

// Chains with a key each (aes_cbc_encrypt_keyed_kernel): every chain has `plain` bytes and becomes
// plain + 16 of ciphertext in place; ONE launch whatever the mix of keys and key lengths.  The
// plan orders the slots so that a wave holds one round count; slot table and wave round counts go
// to d.aes_win, the key table to d.aes_keys, both through the lane's bounce buffer.  The key table
// is zeroed in stream order after the kernel, and when the launch fails after the upload.
int launch_aes_encrypt_keyed(dm_ctx* c, Dev& d, hipStream_t s, const std::vector<CipherKey>& keys,
                             const std::vector<KeyedChain>& chains, uint64_t plain) {
    if (chains.empty()) return DM_OK;
    std::vector<int> rounds(chains.size());
    for (size_t i = 0; i < chains.size(); i++) rounds[i] = keys[chains[i].key].ks.rounds;
    dm_aes_plan::KeyedPlan plan;
    if (!dm_aes_plan::keyed_plan(rounds.data(), rounds.size(), plan))
        return fail(c, DM_ERR_INVALID, "%s", dm_cipher::kKeyLenError);
    const uint64_t nslot = plan.slot.size(), nwave = plan.wave_rounds.size();
    // one upload: the slots, then the waves' round counts
    const uint64_t slot_bytes = nslot * sizeof(dm::AesChainSlot), tab_bytes = slot_bytes + nwave * sizeof(uint32_t);
    std::vector<uint8_t> tab(tab_bytes);
    dm::AesChainSlot* sl = reinterpret_cast<dm::AesChainSlot*>(tab.data());
    for (uint64_t i = 0; i < nslot; i++) {
        const int64_t ch = plan.slot[i];
        sl[i] = ch < 0 ? dm::AesChainSlot{nullptr, 0u, 0u} : dm::AesChainSlot{chains[ch].dev, chains[ch].key, 0u};
    }
    for (uint64_t w = 0; w < nwave; w++) {
        const uint32_t nr = (uint32_t)plan.wave_rounds[w];
        std::memcpy(tab.data() + slot_bytes + 4 * w, &nr, 4);
    }
    std::vector<dm::AesKeyEntry> kt(keys.size());
    for (size_t i = 0; i < keys.size(); i++) {
        std::memcpy(kt[i].w, keys[i].ks.enc, sizeof kt[i].w);
        std::memcpy(kt[i].iv, keys[i].iv, 16);
    }
    const uint64_t key_bytes = kt.size() * sizeof(dm::AesKeyEntry);
    RC_TRY(tables_begin(c, d, tab_bytes + key_bytes + 1024));
    RC_TRY(upload(c, d, s, d.aes_win, tab.data(), tab_bytes));
    const int up = upload(c, d, s, d.aes_keys, kt.data(), key_bytes);
    std::memset(static_cast<void*>(kt.data()), 0, key_bytes);
    hipError_t e = hipSuccess;
    if (up == DM_OK) {
        dm::AesKeyedArgs a{};
        a.slot = reinterpret_cast<const dm::AesChainSlot*>(d.aes_win.u8());
        a.keys = static_cast<const dm::AesKeyEntry*>(d.aes_keys.p);
        a.wave_rounds = reinterpret_cast<const uint32_t*>(d.aes_win.u8() + slot_bytes);
        a.nblk = plain / 16;
        hipLaunchKernelGGL(dm::aes_cbc_encrypt_keyed_kernel, dim3((uint32_t)nwave), dim3(dm::kAesEncThreads), 0, s, a);
        e = hipGetLastError();
    }
    // round keys do not outlive the launch in device memory (a failed upload may have copied some)
    hipError_t z = hipSuccess;
    if (d.aes_keys.p) z = hipMemsetAsync(d.aes_keys.p, 0, key_bytes, s);
    RC_TRY(up);
    HIP_TRY(e);
    HIP_TRY(z);
    return DM_OK;
}

// A chain of a keyed decrypt: cipher_bytes at in -> cipher_bytes - 16 of plaintext at out, under keys[key].
struct KeyedDChain {
    const uint8_t* in;
    uint8_t* out;
    uint32_t key;
};

// Chains with a key each (aes_cbc_decrypt_keyed_kernel): every chain has cipher_bytes of ciphertext;
// ONE launch whatever the mix of keys and key lengths, pad_ok[chain] on the device.  The chain table
// goes to d.aes_win, the key table (the equivalent-inverse-cipher round keys) to d.aes_keys, both
// through the lane's bounce buffer; the key table is zeroed in stream order after the kernel, and
// when the launch fails after the upload, as launch_aes_encrypt_keyed does.
int launch_aes_decrypt_keyed(dm_ctx* c, Dev& d, hipStream_t s, const std::vector<CipherKey>& keys,
                             const std::vector<KeyedDChain>& chains, uint64_t cipher_bytes, uint8_t* pad_ok) {
    if (chains.empty()) return DM_OK;
    if (chains.size() > 0xffffffffull || cipher_bytes / 16 > 0xffffffffull)   // the kernel counts both in 32 bits
        return fail(c, DM_ERR_INVALID, "keyed decrypt: at most 2^32 - 1 chains of at most 2^32 - 1 blocks");
    std::vector<dm::AesDChain> tab(chains.size());
    for (size_t i = 0; i < chains.size(); i++)
        tab[i] = dm::AesDChain{chains[i].in, chains[i].out, chains[i].key, (uint32_t)keys[chains[i].key].ks.rounds, 0};
    std::vector<dm::AesKeyEntry> kt(keys.size());
    for (size_t i = 0; i < keys.size(); i++) {
        std::memcpy(kt[i].w, keys[i].ks.dec, sizeof kt[i].w);
        std::memcpy(kt[i].iv, keys[i].iv, 16);
    }
    const uint64_t tab_bytes = tab.size() * sizeof(dm::AesDChain), key_bytes = kt.size() * sizeof(dm::AesKeyEntry);
    const int tb = tables_begin(c, d, tab_bytes + key_bytes + 1024);
    if (tb != DM_OK) std::memset(static_cast<void*>(kt.data()), 0, key_bytes);
    RC_TRY(tb);
    int up = upload(c, d, s, d.aes_win, tab.data(), tab_bytes);
    const bool keys_sent = up == DM_OK;
    if (up == DM_OK) up = upload(c, d, s, d.aes_keys, kt.data(), key_bytes);
    std::memset(static_cast<void*>(kt.data()), 0, key_bytes);
    hipError_t e = hipSuccess;
    if (up == DM_OK) {
        const uint64_t nblk = cipher_bytes / 16;
        const dim3 grid = rs_grid(d, nblk, chains.size()), block(dm::kAesDecThreads);
        hipLaunchKernelGGL(dm::aes_cbc_decrypt_keyed_kernel, grid, block, 0, s,
                           static_cast<const dm::AesDChain*>(d.aes_win.p), static_cast<const dm::AesKeyEntry*>(d.aes_keys.p),
                           (uint32_t)chains.size(), (uint32_t)nblk, pad_ok);
        e = hipGetLastError();
    }
    // round keys do not outlive the launch in device memory (a failed upload may have copied some)
    hipError_t z = hipSuccess;
    if (keys_sent && d.aes_keys.p) z = hipMemsetAsync(d.aes_keys.p, 0, key_bytes, s);
    RC_TRY(up);
    HIP_TRY(e);
    HIP_TRY(z);
    return DM_OK;
}

}  // namespace

extern "C" {

int dm_aes_cbc_decrypt_keyed_device_async(dm_ctx* ctx, const dm_aes_key* keys, uint64_t nkeys, const dm_aes_dchain* chains,
                                          uint64_t nchain, uint64_t cipher_bytes, void* dev_pad_ok, void* stream) {
    if (!ctx || (nkeys && !keys)) return bad_arg();
    const int g = device_of(ctx, nchain && chains ? chains[0].dev_in : nullptr);
    CallLock lk(ctx, g, kReserved);
    dm_ctx* c = ctx;
    std::vector<CipherKey> ks(nkeys);
    for (uint64_t i = 0; i < nkeys; i++) {
        if (!keys[i].key || !dm_aes::expand_key(static_cast<const uint8_t*>(keys[i].key), keys[i].key_len, ks[i].ks))
            return fail(c, DM_ERR_INVALID, "key %llu: %s", (unsigned long long)i, dm_cipher::kKeyLenError);
        cipher_set_iv(ks[i], keys[i].iv);
    }
    if (nchain == 0) return DM_OK;
    if (!chains || !dev_pad_ok)
        return fail(c, DM_ERR_INVALID, "dm_aes_cbc_decrypt_keyed_device_async: null chains or verdict buffer");
    if (cipher_bytes % 16 || cipher_bytes < 32)
        return fail(c, DM_ERR_INVALID,
                    "dm_aes_cbc_decrypt_keyed_device_async: need cipher_bytes %% 16 == 0 and cipher_bytes >= 32");
    std::vector<KeyedDChain> ch(nchain);
    for (uint64_t i = 0; i < nchain; i++) {
        const dm_aes_dchain& x = chains[i];
        if (!x.dev_in || !x.dev_out || !is_aligned16(x.dev_in) || !is_aligned16(x.dev_out) || x.key_index >= nkeys)
            return fail(c, DM_ERR_INVALID,
                        "dm_aes_cbc_decrypt_keyed_device_async: chain %llu needs 16-byte aligned in and out and a key "
                        "index below %llu", (unsigned long long)i, (unsigned long long)nkeys);
        ch[i] = KeyedDChain{static_cast<const uint8_t*>(x.dev_in), static_cast<uint8_t*>(x.dev_out), x.key_index};
    }
    Dev& d = c->devs[g];
    hipStream_t s = pick_stream(d, stream);
    RC_TRY(begin_call(c, d, s));
    return launch_aes_decrypt_keyed(c, d, s, ks, ch, cipher_bytes, static_cast<uint8_t*>(dev_pad_ok));
}

int dm_aes_cbc_encrypt_keyed_device_async(dm_ctx* ctx, const dm_aes_key* keys, uint64_t nkeys, const dm_aes_chain* chains,
                                          uint64_t nchain, uint64_t plain, void* stream) {
    if (!ctx || (nkeys && !keys)) return bad_arg();
    const int g = device_of(ctx, nchain && chains ? chains[0].dev : nullptr);
    CallLock lk(ctx, g, kReserved);
    dm_ctx* c = ctx;
    std::vector<CipherKey> ks(nkeys);
    for (uint64_t i = 0; i < nkeys; i++) {
        if (!keys[i].key || !dm_aes::expand_key(static_cast<const uint8_t*>(keys[i].key), keys[i].key_len, ks[i].ks))
            return fail(c, DM_ERR_INVALID, "key %llu: %s", (unsigned long long)i, dm_cipher::kKeyLenError);
        cipher_set_iv(ks[i], keys[i].iv);
    }
    if (nchain == 0) return DM_OK;
    if (!chains) return fail(c, DM_ERR_INVALID, "dm_aes_cbc_encrypt_keyed_device_async: null chains");
    if (plain % 16)
        return fail(c, DM_ERR_INVALID, "dm_aes_cbc_encrypt_keyed_device_async: need plain %% 16 == 0");
    std::vector<KeyedChain> ch(nchain);
    for (uint64_t i = 0; i < nchain; i++) {
        if (!chains[i].dev || !is_aligned16(chains[i].dev) || chains[i].key_index >= nkeys)
            return fail(c, DM_ERR_INVALID,
                        "dm_aes_cbc_encrypt_keyed_device_async: chain %llu needs a 16-byte aligned buffer and a key "
                        "index below %llu", (unsigned long long)i, (unsigned long long)nkeys);
        ch[i] = KeyedChain{static_cast<uint8_t*>(chains[i].dev), chains[i].key_index};
    }
    Dev& d = c->devs[g];
    hipStream_t s = pick_stream(d, stream);
    RC_TRY(begin_call(c, d, s));
    return launch_aes_encrypt_keyed(c, d, s, ks, ch, plain);
}

int dm_aes_cbc_decrypt_windows_device_async(dm_ctx* ctx, const void* key, uint64_t key_len, const uint8_t iv[16],
                                            const dm_aes_window* windows, uint64_t nwin, void* dev_pad_ok, void* stream) {
    if (!ctx || !key || !iv) return bad_arg();
    const int g = device_of(ctx, nwin && windows ? windows[0].in : nullptr);
    CallLock lk(ctx, g, kReserved);
    dm_ctx* c = ctx;
    CipherKey k;
    if (!dm_aes::expand_key(static_cast<const uint8_t*>(key), key_len, k.ks))
        return fail(c, DM_ERR_INVALID, "%s", dm_cipher::kKeyLenError);
    cipher_set_iv(k, iv);
    if (nwin == 0) return DM_OK;
    if (!windows) return fail(c, DM_ERR_INVALID, "dm_aes_cbc_decrypt_windows_device_async: null windows");
    std::vector<dm::AesWindow> win(nwin);
    for (uint64_t w = 0; w < nwin; w++) {
        const dm_aes_window& x = windows[w];
        const bool pad = x.check_pad != 0;
        if (!x.in || !x.out || !is_aligned16(x.in) || !is_aligned16(x.prev) || !is_aligned16(x.out) ||
            x.nblk < (pad ? 2u : 1u) || (pad && !dev_pad_ok))
            return fail(c, DM_ERR_INVALID,
                        "dm_aes_cbc_decrypt_windows_device_async: window %llu needs 16-byte aligned in, prev and out, "
                        "nblk >= 1 (>= 2 and a verdict buffer with check_pad)", (unsigned long long)w);
        win[w] = dm::AesWindow{static_cast<const uint8_t*>(x.in), static_cast<const uint8_t*>(x.prev),
                               static_cast<uint8_t*>(x.out), x.nblk, pad ? 1u : 0u, 0u};
    }
    Dev& d = c->devs[g];
    hipStream_t s = pick_stream(d, stream);
    RC_TRY(begin_call(c, d, s));
    return launch_aes_decrypt_windows(c, d, s, k, win, static_cast<uint8_t*>(dev_pad_ok));
}

int dm_aes_cbc_encrypt_device_async(dm_ctx* ctx, const void* key, uint64_t key_len, const uint8_t iv[16], void* dev,
                                    uint64_t stride, uint64_t plain, uint64_t nseg, void* stream) {
    if (!ctx || !key || !iv) return bad_arg();
    const int g = device_of(ctx, dev);
    CallLock lk(ctx, g, kReserved);
    dm_ctx* c = ctx;
    CipherKey k;
    if (!dm_aes::expand_key(static_cast<const uint8_t*>(key), key_len, k.ks))
        return fail(c, DM_ERR_INVALID, "%s", dm_cipher::kKeyLenError);
    cipher_set_iv(k, iv);
    if (nseg == 0) return DM_OK;
    if (!dev || !is_aligned16(dev) || plain % 16 || stride % 16 || plain + 16 > stride)
        return fail(c, DM_ERR_INVALID,
                    "dm_aes_cbc_encrypt_device_async: need a 16-byte aligned buffer and stride, plain %% 16 == 0 and "
                    "plain + 16 <= stride");
    Dev& d = c->devs[g];
    hipStream_t s = pick_stream(d, stream);
    RC_TRY(begin_call(c, d, s));
    HIP_TRY(launch_aes_encrypt(s, k, static_cast<uint8_t*>(dev), stride, plain, nseg));
    return DM_OK;
}

int dm_aes_cbc_encrypt_range_device_async(dm_ctx* ctx, const void* key, uint64_t key_len, const uint8_t iv[16],
                                          void* dev, uint64_t stride, uint64_t plain, uint64_t nseg, uint64_t blk_lo,
                                          uint64_t blk_hi, void* stream) {
    if (!ctx || !key || !iv) return bad_arg();
    const int g = device_of(ctx, dev);
    CallLock lk(ctx, g, kReserved);
    dm_ctx* c = ctx;
    CipherKey k;
    if (!dm_aes::expand_key(static_cast<const uint8_t*>(key), key_len, k.ks))
        return fail(c, DM_ERR_INVALID, "%s", dm_cipher::kKeyLenError);
    cipher_set_iv(k, iv);
    if (nseg == 0) return DM_OK;
    if (!dev || !is_aligned16(dev) || plain % 16 || stride % 16 || plain + 16 > stride)
        return fail(c, DM_ERR_INVALID,
                    "dm_aes_cbc_encrypt_range_device_async: need a 16-byte aligned buffer and stride, plain %% 16 == 0 "
                    "and plain + 16 <= stride");
    if (blk_lo >= blk_hi || blk_hi > plain / 16)
        return fail(c, DM_ERR_INVALID,
                    "dm_aes_cbc_encrypt_range_device_async: blocks [%llu, %llu) are not a range of the %llu of a chain",
                    (unsigned long long)blk_lo, (unsigned long long)blk_hi, (unsigned long long)(plain / 16));
    Dev& d = c->devs[g];
    hipStream_t s = pick_stream(d, stream);
    RC_TRY(begin_call(c, d, s));
    HIP_TRY(launch_aes_encrypt_range(s, k, static_cast<uint8_t*>(dev), stride, plain, nseg, blk_lo, blk_hi));
    return DM_OK;
}

int dm_aes_cbc_decrypt_device_async(dm_ctx* ctx, const void* key, uint64_t key_len, const uint8_t iv[16],
                                    const void* dev_in, uint64_t in_stride, uint64_t cipher_bytes, uint64_t nseg,
                                    void* dev_out, uint64_t out_stride, void* dev_pad_ok, void* stream) {
    if (!ctx || !key || !iv) return bad_arg();
    const int g = device_of(ctx, dev_in);
    CallLock lk(ctx, g, kReserved);
    dm_ctx* c = ctx;
    CipherKey k;
    if (!dm_aes::expand_key(static_cast<const uint8_t*>(key), key_len, k.ks))
        return fail(c, DM_ERR_INVALID, "%s", dm_cipher::kKeyLenError);
    cipher_set_iv(k, iv);
    if (nseg == 0) return DM_OK;
    if (!dev_in || !dev_out || !dev_pad_ok || !is_aligned16(dev_in) || !is_aligned16(dev_out) || cipher_bytes % 16 ||
        cipher_bytes < 32 || in_stride % 16 || out_stride % 16 || in_stride < cipher_bytes ||
        out_stride < cipher_bytes - 16)
        return fail(c, DM_ERR_INVALID,
                    "dm_aes_cbc_decrypt_device_async: need 16-byte aligned buffers and strides, cipher_bytes %% 16 == 0, "
                    "cipher_bytes >= 32 and strides that hold a segment");
    Dev& d = c->devs[g];
    hipStream_t s = pick_stream(d, stream);
    RC_TRY(begin_call(c, d, s));
    HIP_TRY(launch_aes_decrypt(d, s, k, static_cast<const uint8_t*>(dev_in), in_stride, cipher_bytes, nseg,
                               static_cast<uint8_t*>(dev_out), out_stride, static_cast<uint8_t*>(dev_pad_ok)));
    return DM_OK;
}

}  // extern "C"
