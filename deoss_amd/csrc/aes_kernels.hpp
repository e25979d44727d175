// aes_kernels.hpp -- gfx950 AES-CBC for the cipher branch of FullProcessing / Retrievefile
// (cipher_scheme.hpp says how the SDK uses it).  Included by merkle_capi.hip only (cipher_capi.inl).
//
// Both kernels are T-table AES (FIPS-197 §5; the decrypt side is the equivalent inverse cipher of
// §5.3.5): SubBytes + ShiftRows + MixColumns of one state byte is one 32-bit table lookup, a round
// is 16 lookups and 16 xors.  The tables are generated at compile time (aes_host.hpp), copied to
// LDS at kernel start (4 x 1 KiB rotations of one table + the S-box for the last round); the round
// keys are expanded on the host and arrive as kernel arguments.
//
//   aes_cbc_decrypt_kernel  P_i = D(C_i) ^ C_{i-1} is parallel over blocks: one lane per 16-byte
//       block, x over a segment's blocks and y over segments (launch_rs's grid), 16-byte loads,
//       non-temporal 16-byte stores, out of place and compacting (the padding block is checked,
//       not written).
//   aes_cbc_decrypt_window_kernel  the same per block, over a table of windows that may start in
//       the middle of a chain (each names its predecessor block) and differ in length: the ranged
//       restore (range_capi.inl).
//   aes_cbc_encrypt_kernel  C_i = E(P_i ^ C_{i-1}) is one serial chain per segment.  FOUR lanes (a
//       DPP quad) carry a chain, lane j the state column j: it looks its own four bytes up in the
//       four tables, and ShiftRows is three quad_perm reads of the neighbours' lookups (xor-ed on
//       the way), so a round is 4 address extracts, 4 independent ds_read_b32, 4 xors.  The state
//       never leaves registers; the plaintext is loaded kAesDepth blocks ahead.  16 chains per
//       wave, one wave per workgroup: 256 segments spread over 16 CUs' SIMDs.
//       Latency-bound like the SHA-256 chains: a throughput path.
//   aes_cbc_encrypt_range_kernel  the same chains, blocks [blk_lo, blk_hi) only: the chaining value
//       is read back from the buffer, so the striped file path (fullproc_capi.inl) encrypts each
//       stripe as it lands and the SHA-256 chains follow one stripe behind.
//   aes_cbc_encrypt_keyed_kernel  the same chains with a key per chain: chains and keys come from
//       tables in device memory, a wave holds chains of one round count (aes_keyed_plan.hpp) and
//       branches once into the loop unrolled for it, so ONE launch encrypts a batch of different
//       clients' uploads (dm_process_cipher_batch, the batcher) in the time of its longest chain.
//   aes_cbc_decrypt_keyed_kernel  aes_cbc_decrypt_kernel's block work with a key per chain: chain
//       descriptors (in, out, key index, round count) and keys come from tables in device memory
//       by scalar loads, once per chain, the key again only when its index changes, so ONE launch
//       decrypts a batch of different clients' downloads (dm_restore_batch).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aes_host.hpp"

namespace dm {

constexpr int kAesDecThreads = 256;
constexpr int kAesEncThreads = 64;    // one wave: 16 chains x 4 lanes
constexpr int kAesLanesPerChain = 4;
constexpr int kAesDepth = 8;          // plaintext blocks in flight ahead of the chain
constexpr uint32_t kAesPadWord = 0x10101010u;   // PKCS#7 padding of a whole block

struct AesKey {
    uint32_t w[dm_aes::kMaxKeyWords];   // 240 bytes, little-endian column words, round-major
};

struct AesEncArgs {
    AesKey rk;
    uint32_t iv[4];
    uint8_t* dev;        // segment s: nblk plaintext blocks at dev + s * stride, overwritten by nblk + 1 ciphertext blocks
    uint64_t stride;
    uint64_t nblk;
    uint64_t nseg;
};

struct AesDecArgs {
    AesKey rk;           // equivalent-inverse-cipher keys
    uint32_t iv[4];
    const uint8_t* in;   // segment s: nblk ciphertext blocks at in + s * in_stride
    uint64_t in_stride;
    uint64_t nblk;       // >= 2: the last one is the padding block
    uint64_t nseg;
    uint8_t* out;        // segment s: nblk - 1 plaintext blocks at out + s * out_stride
    uint64_t out_stride;
    uint8_t* pad_ok;     // [nseg]: 1 iff the last block decrypts to sixteen 0x10 bytes
};

__device__ __constant__ static const dm_aes::Tables kAesTables{};

__device__ __forceinline__ uint32_t aes_rotl(uint32_t x, uint32_t n) { return (x << n) | (x >> (32 - n)); }

// tab[r * 256 + a] = rotl(t0[a], 8 r) for r < 4; tab[1024 + a] = the S-box byte in all four bytes.
template <int THREADS>
__device__ __forceinline__ void aes_fill_lds(uint32_t* tab, const uint32_t* t0, const uint8_t* sb) {
    for (uint32_t t = threadIdx.x; t < 256; t += THREADS) {
        const uint32_t e = t0[t];
        tab[t] = e;
        tab[256 + t] = aes_rotl(e, 8);
        tab[512 + t] = aes_rotl(e, 16);
        tab[768 + t] = aes_rotl(e, 24);
        tab[1024 + t] = (uint32_t)sb[t] * 0x01010101u;
    }
    __syncthreads();
}

// Lane i of a quad reads lane (i + R) & 3's value.
template <int R>
__device__ __forceinline__ uint32_t aes_quad_rot(uint32_t v) {
    constexpr int ctrl = ((0 + R) & 3) | (((1 + R) & 3) << 2) | (((2 + R) & 3) << 4) | (((3 + R) & 3) << 6);
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, 0xf, 0xf, true);
}

// One block on a quad: x = this lane's column of (plaintext ^ chain), rk = its column of every
// round key.  Row r of the output column i comes from input column i + r (ShiftRows).
template <int NR>
__device__ __forceinline__ uint32_t aes_encrypt_quad(uint32_t x, const uint32_t (&rk)[NR + 1], const uint32_t* tab) {
    x ^= rk[0];
#pragma unroll
    for (int r = 1; r < NR; r++) {
        const uint32_t t0 = tab[x & 0xffu];
        const uint32_t t1 = tab[256 + ((x >> 8) & 0xffu)];
        const uint32_t t2 = tab[512 + ((x >> 16) & 0xffu)];
        const uint32_t t3 = tab[768 + (x >> 24)];
        x = t0 ^ aes_quad_rot<1>(t1) ^ aes_quad_rot<2>(t2) ^ aes_quad_rot<3>(t3) ^ rk[r];
    }
    const uint32_t u0 = tab[1024 + (x & 0xffu)] & 0x000000ffu;
    const uint32_t u1 = tab[1024 + ((x >> 8) & 0xffu)] & 0x0000ff00u;
    const uint32_t u2 = tab[1024 + ((x >> 16) & 0xffu)] & 0x00ff0000u;
    const uint32_t u3 = tab[1024 + (x >> 24)] & 0xff000000u;
    return u0 ^ aes_quad_rot<1>(u1) ^ aes_quad_rot<2>(u2) ^ aes_quad_rot<3>(u3) ^ rk[NR];
}

// Grid: ceil(nseg / 16) workgroups of one wave.  Every segment has the same block count, so the
// loop bounds are uniform over the wave; a quad is wholly inside or outside nseg.
template <int NR>
__global__ __launch_bounds__(kAesEncThreads)
void aes_cbc_encrypt_kernel(AesEncArgs a) {
    __shared__ uint32_t tab[5 * 256];
    aes_fill_lds<kAesEncThreads>(tab, kAesTables.te0, kAesTables.sbox);
    const uint32_t j = threadIdx.x & 3u;
    const uint64_t chain = ((uint64_t)blockIdx.x * kAesEncThreads + threadIdx.x) / kAesLanesPerChain;
    if (chain >= a.nseg) return;
    uint32_t rk[NR + 1];
#pragma unroll
    for (int r = 0; r <= NR; r++) {
        const uint32_t k01 = j & 1u ? a.rk.w[4 * r + 1] : a.rk.w[4 * r];
        const uint32_t k23 = j & 1u ? a.rk.w[4 * r + 3] : a.rk.w[4 * r + 2];
        rk[r] = j & 2u ? k23 : k01;
    }
    const uint32_t iv01 = j & 1u ? a.iv[1] : a.iv[0], iv23 = j & 1u ? a.iv[3] : a.iv[2];
    uint32_t c = j & 2u ? iv23 : iv01;
    uint32_t* p = reinterpret_cast<uint32_t*>(a.dev + chain * a.stride) + j;   // this lane's column of block 0
    const uint64_t nblk = a.nblk, total = nblk + 1;   // the padding block comes after the data
    uint32_t pf[kAesDepth];
#pragma unroll
    for (int i = 0; i < kAesDepth; i++) pf[i] = (uint64_t)i < nblk ? p[4 * i] : kAesPadWord;
    for (uint64_t b0 = 0; b0 < total; b0 += kAesDepth) {
#pragma unroll
        for (int i = 0; i < kAesDepth; i++) {
            const uint64_t b = b0 + i;
            if (b >= total) break;
            const uint32_t x = pf[i] ^ c;
            // block b + kAesDepth (still plaintext: the chain has written blocks < b only)
            pf[i] = b + kAesDepth < nblk ? p[4 * (b + kAesDepth)] : kAesPadWord;
            c = aes_encrypt_quad<NR>(x, rk, tab);
            p[4 * b] = c;
        }
    }
}

// The chain in pieces: plaintext blocks [blk_lo, blk_hi) of every chain, in place.  CBC resumes from
// the previous ciphertext block alone, and that one is in the buffer (blk_lo - 1; the IV at 0), so
// a launch carries no state to the next.  Blocks at or beyond blk_hi are neither read nor written
// -- in the striped file path they are still on the copy stream -- but for the padding block, which
// the launch that ends the data (blk_hi == nblk) appends.  Grid and layout as above.
struct AesEncRangeArgs {
    AesEncArgs e;
    uint64_t blk_lo, blk_hi;   // blk_lo < blk_hi <= e.nblk
};

template <int NR>
__global__ __launch_bounds__(kAesEncThreads)
void aes_cbc_encrypt_range_kernel(AesEncRangeArgs ra) {
    __shared__ uint32_t tab[5 * 256];
    aes_fill_lds<kAesEncThreads>(tab, kAesTables.te0, kAesTables.sbox);
    const AesEncArgs& a = ra.e;
    const uint32_t j = threadIdx.x & 3u;
    const uint64_t chain = ((uint64_t)blockIdx.x * kAesEncThreads + threadIdx.x) / kAesLanesPerChain;
    if (chain >= a.nseg) return;
    uint32_t rk[NR + 1];
#pragma unroll
    for (int r = 0; r <= NR; r++) {
        const uint32_t k01 = j & 1u ? a.rk.w[4 * r + 1] : a.rk.w[4 * r];
        const uint32_t k23 = j & 1u ? a.rk.w[4 * r + 3] : a.rk.w[4 * r + 2];
        rk[r] = j & 2u ? k23 : k01;
    }
    uint32_t* p = reinterpret_cast<uint32_t*>(a.dev + chain * a.stride) + j;   // this lane's column of block 0
    const uint64_t lo = ra.blk_lo, hi = ra.blk_hi;
    const uint64_t end = hi == a.nblk ? hi + 1 : hi;   // the padding block comes after the last data block
    const uint32_t iv01 = j & 1u ? a.iv[1] : a.iv[0], iv23 = j & 1u ? a.iv[3] : a.iv[2];
    uint32_t c = j & 2u ? iv23 : iv01;
    if (lo) c = p[4 * (lo - 1)];
    uint32_t pf[kAesDepth];
#pragma unroll
    for (int i = 0; i < kAesDepth; i++) pf[i] = lo + i < hi ? p[4 * (lo + i)] : kAesPadWord;
    for (uint64_t b0 = lo; b0 < end; b0 += kAesDepth) {
#pragma unroll
        for (int i = 0; i < kAesDepth; i++) {
            const uint64_t b = b0 + i;
            if (b >= end) break;
            const uint32_t x = pf[i] ^ c;
            // block b + kAesDepth (still plaintext: the chain has written blocks < b only); none at or past hi
            pf[i] = b + kAesDepth < hi ? p[4 * (b + kAesDepth)] : kAesPadWord;
            c = aes_encrypt_quad<NR>(x, rk, tab);
            p[4 * b] = c;
        }
    }
}

__device__ __forceinline__ uint4 aes_load16(const uint8_t* p) { return *reinterpret_cast<const uint4*>(p); }

// The equivalent inverse cipher on a whole block in one lane.  Row r of output column i comes from
// input column i - r (InvShiftRows).
template <int NR>
__device__ __forceinline__ uint4 aes_decrypt_block(uint4 cblk, const AesKey& dk, const uint32_t* tab) {
    uint32_t s[4] = {cblk.x ^ dk.w[0], cblk.y ^ dk.w[1], cblk.z ^ dk.w[2], cblk.w ^ dk.w[3]};
#pragma unroll
    for (int r = 1; r < NR; r++) {
        uint32_t t[4];
#pragma unroll
        for (int i = 0; i < 4; i++)
            t[i] = tab[s[i] & 0xffu] ^ tab[256 + ((s[(i + 3) & 3] >> 8) & 0xffu)] ^
                   tab[512 + ((s[(i + 2) & 3] >> 16) & 0xffu)] ^ tab[768 + (s[(i + 1) & 3] >> 24)] ^ dk.w[4 * r + i];
#pragma unroll
        for (int i = 0; i < 4; i++) s[i] = t[i];
    }
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
        o[i] = (tab[1024 + (s[i] & 0xffu)] & 0x000000ffu) ^ (tab[1024 + ((s[(i + 3) & 3] >> 8) & 0xffu)] & 0x0000ff00u) ^
               (tab[1024 + ((s[(i + 2) & 3] >> 16) & 0xffu)] & 0x00ff0000u) ^
               (tab[1024 + (s[(i + 1) & 3] >> 24)] & 0xff000000u) ^ dk.w[4 * NR + i];
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// Grid: x strides over a segment's blocks, y over segments (rs_grid).
template <int NR>
__global__ __launch_bounds__(kAesDecThreads)
void aes_cbc_decrypt_kernel(AesDecArgs a) {
    __shared__ uint32_t tab[5 * 256];
    aes_fill_lds<kAesDecThreads>(tab, kAesTables.td0, kAesTables.inv);
    const uint64_t ustride = (uint64_t)gridDim.x * kAesDecThreads;
    const uint4 iv = make_uint4(a.iv[0], a.iv[1], a.iv[2], a.iv[3]);
    for (uint64_t seg = blockIdx.y; seg < a.nseg; seg += gridDim.y) {
        const uint8_t* in = a.in + seg * a.in_stride;
        uint8_t* out = a.out + seg * a.out_stride;
        uint64_t u = (uint64_t)blockIdx.x * kAesDecThreads + threadIdx.x;
        // register double buffer: the next block's loads are in flight while this one is decrypted
        uint4 nc = iv, np = iv;
        if (u < a.nblk) {
            nc = aes_load16(in + u * 16);
            if (u) np = aes_load16(in + (u - 1) * 16);
        }
        for (; u < a.nblk; u += ustride) {
            const uint4 cblk = nc, prev = np;
            if (u + ustride < a.nblk) {
                nc = aes_load16(in + (u + ustride) * 16);
                np = aes_load16(in + (u + ustride - 1) * 16);
            }
            uint4 x = aes_decrypt_block<NR>(cblk, a.rk, tab);
            x.x ^= prev.x;
            x.y ^= prev.y;
            x.z ^= prev.z;
            x.w ^= prev.w;
            if (u + 1 < a.nblk)
                rs_store(out + u * 16, x);
            else
                a.pad_ok[seg] = (x.x == kAesPadWord && x.y == kAesPadWord && x.z == kAesPadWord && x.w == kAesPadWord) ? 1 : 0;
        }
    }
}

// ---- windows: decryption that starts in the middle of a chain (ranged restore, range_capi.inl) ----

// One window of a CBC chain: nblk ciphertext blocks at `in`, their plaintext to `out`.  P_i needs
// C_{i-1} only, so a window needs its predecessor block and nothing else of the chain; that block
// has an address of its own (it may lie in another buffer), null = the IV.
struct AesWindow {
    const uint8_t* in;
    const uint8_t* prev;
    uint8_t* out;
    uint64_t nblk;        // >= 1; >= 2 with check_pad
    uint32_t check_pad;   // the last block is a padding block: its verdict goes to pad_ok[w], it is not stored
    uint32_t pad_;
};

struct AesWinArgs {
    AesKey rk;              // equivalent-inverse-cipher keys
    uint32_t iv[4];
    const AesWindow* win;   // [nwin], device memory
    uint64_t nwin;
    uint8_t* pad_ok;        // [nwin]; written for check_pad windows only
};

// Grid: x strides over a window's blocks, y over windows (rs_grid for the longest window; a shorter
// one leaves lanes idle).  One lane per block as aes_cbc_decrypt_kernel; the descriptor is uniform
// over the workgroup and read once per window.
template <int NR>
__global__ __launch_bounds__(kAesDecThreads)
void aes_cbc_decrypt_window_kernel(AesWinArgs a) {
    __shared__ uint32_t tab[5 * 256];
    aes_fill_lds<kAesDecThreads>(tab, kAesTables.td0, kAesTables.inv);
    const uint64_t ustride = (uint64_t)gridDim.x * kAesDecThreads;
    const uint4 iv = make_uint4(a.iv[0], a.iv[1], a.iv[2], a.iv[3]);
    for (uint64_t w = blockIdx.y; w < a.nwin; w += gridDim.y) {
        const AesWindow d = a.win[w];
        const uint64_t nstore = d.nblk - (d.check_pad ? 1 : 0);
        uint64_t u = (uint64_t)blockIdx.x * kAesDecThreads + threadIdx.x;
        // register double buffer: the next stride's loads are in flight while this block is decrypted
        uint4 nc = iv, np = iv;
        if (u < d.nblk) {
            nc = aes_load16(d.in + u * 16);
            if (u)
                np = aes_load16(d.in + (u - 1) * 16);
            else if (d.prev)
                np = aes_load16(d.prev);
        }
        for (; u < d.nblk; u += ustride) {
            const uint4 cblk = nc, prev = np;
            if (u + ustride < d.nblk) {
                nc = aes_load16(d.in + (u + ustride) * 16);
                np = aes_load16(d.in + (u + ustride - 1) * 16);
            }
            uint4 x = aes_decrypt_block<NR>(cblk, a.rk, tab);
            x.x ^= prev.x;
            x.y ^= prev.y;
            x.z ^= prev.z;
            x.w ^= prev.w;
            if (u < nstore)
                rs_store(d.out + u * 16, x);
            else
                a.pad_ok[w] = (x.x == kAesPadWord && x.y == kAesPadWord && x.z == kAesPadWord && x.w == kAesPadWord) ? 1 : 0;
        }
    }
}

// ---- a key per chain: encrypted uploads of different clients in ONE launch (dm_process_cipher_batch) ----

// One chain of a keyed launch: nblk plaintext blocks at dev, overwritten by nblk + 1 ciphertext
// blocks under key table entry `key`.  dev == nullptr: an empty slot (aes_keyed_plan.hpp pads a
// round-count group to whole waves with them).
struct AesChainSlot {
    uint8_t* dev;
    uint32_t key;
    uint32_t pad_;
};
static_assert(sizeof(AesChainSlot) == 16, "one 16-byte descriptor per slot");

// One key of a keyed launch: the encryption round keys (round-major column words, as AesKey) and
// the IV.  The only place round keys sit in device memory: the host zeroes the table in stream
// order right after the launch (launch_aes_encrypt_keyed).
struct AesKeyEntry {
    uint32_t w[dm_aes::kMaxKeyWords];
    uint32_t iv[4];
};
static_assert(sizeof(AesKeyEntry) == 256, "60 round-key words + 4 IV words");

struct AesKeyedArgs {
    const AesChainSlot* slot;      // [16 * nwave], device memory
    const AesKeyEntry* keys;       // device memory
    const uint32_t* wave_rounds;   // [nwave]: 10, 12 or 14, the round count of every chain of the wave
    uint64_t nblk;                 // plaintext blocks of every chain
};

// The chain of aes_cbc_encrypt_kernel with the key read from the table: lane j loads its column
// w[4 r + j] of every round key and its IV word once, into registers.
template <int NR>
__device__ __forceinline__ void aes_keyed_chain(uint32_t* p, const AesKeyEntry* k, uint32_t j, uint64_t nblk,
                                                const uint32_t* tab) {
    uint32_t rk[NR + 1];
#pragma unroll
    for (int r = 0; r <= NR; r++) rk[r] = k->w[4 * r + j];
    uint32_t c = k->iv[j];
    const uint64_t total = nblk + 1;   // the padding block comes after the data
    uint32_t pf[kAesDepth];
#pragma unroll
    for (int i = 0; i < kAesDepth; i++) pf[i] = (uint64_t)i < nblk ? p[4 * i] : kAesPadWord;
    for (uint64_t b0 = 0; b0 < total; b0 += kAesDepth) {
#pragma unroll
        for (int i = 0; i < kAesDepth; i++) {
            const uint64_t b = b0 + i;
            if (b >= total) break;
            const uint32_t x = pf[i] ^ c;
            // block b + kAesDepth (still plaintext: the chain has written blocks < b only)
            pf[i] = b + kAesDepth < nblk ? p[4 * (b + kAesDepth)] : kAesPadWord;
            c = aes_encrypt_quad<NR>(x, rk, tab);
            p[4 * b] = c;
        }
    }
}

// Grid: one workgroup of one wave per 16 slots.  Every chain has nblk blocks and every chain of a
// wave the same round count (read once, uniform: a scalar branch into one of three unrolled loops),
// so the loop bounds are uniform over the wave; a quad is wholly a chain or wholly an empty slot.
__global__ __launch_bounds__(kAesEncThreads)
void aes_cbc_encrypt_keyed_kernel(AesKeyedArgs a) {
    __shared__ uint32_t tab[5 * 256];
    aes_fill_lds<kAesEncThreads>(tab, kAesTables.te0, kAesTables.sbox);
    const uint32_t j = threadIdx.x & 3u;
    const uint32_t nr = a.wave_rounds[blockIdx.x];
    const AesChainSlot sl = a.slot[(uint64_t)blockIdx.x * (kAesEncThreads / kAesLanesPerChain) + threadIdx.x / kAesLanesPerChain];
    if (!sl.dev) return;
    uint32_t* p = reinterpret_cast<uint32_t*>(sl.dev) + j;   // this lane's column of block 0
    const AesKeyEntry* k = a.keys + sl.key;
    if (nr == 10)
        aes_keyed_chain<10>(p, k, j, a.nblk, tab);
    else if (nr == 12)
        aes_keyed_chain<12>(p, k, j, a.nblk, tab);
    else
        aes_keyed_chain<14>(p, k, j, a.nblk, tab);
}

// ---- a key per chain, decrypt: different clients' downloads in ONE launch (dm_restore_batch) ----

// One chain of a keyed decrypt: nblk ciphertext blocks at `in`, nblk - 1 plaintext blocks to `out`
// (anywhere: no common stride, so one object's pieces join back to back while another's lie
// elsewhere) under key table entry `key`, whose round count the host repeats here.
struct AesDChain {
    const uint8_t* in;
    uint8_t* out;
    uint32_t key;
    uint32_t rounds;   // 10, 12 or 14
    uint64_t pad_;
};
static_assert(sizeof(AesDChain) == 32, "one 32-byte descriptor per chain");

// Addresses read out of a table have no address space the compiler can see; without these casts
// they become flat accesses (seen in the disassembly), which by the ISA's rules count against the
// LDS lookups' wait counter as well -- reasoned from the ISA, the cost was not measured.
typedef uint32_t aes_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) aes_u32x4 aes_gu32x4;

__device__ __forceinline__ uint4 aes_gload16(const uint8_t* p) {
    const aes_u32x4 v = *(const aes_gu32x4*)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ void aes_gstore16(uint8_t* p, uint4 v) {   // non-temporal, as rs_store
    const aes_u32x4 w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, (aes_gu32x4*)p);
}

// The block loop of aes_cbc_decrypt_kernel for one chain: one lane per block, the next stride's
// loads in flight, the padding block checked by the lane that owns it and not stored.  Only the lane
// of block 0 needs the IV: it loads it from the key entry, the others their predecessor block.
template <int NR>
__device__ __forceinline__ void aes_dkeyed_blocks(const uint8_t* in, uint8_t* out, uint32_t nblk, uint32_t ustride,
                                                  const AesKey& dk, const uint32_t* iv, const uint32_t* tab,
                                                  uint8_t* pad_ok) {
    uint32_t u = blockIdx.x * kAesDecThreads + threadIdx.x;
    if (u >= nblk) return;
    // per-lane cursors: the chain's base addresses need not outlive this line in scalar registers
    const uint8_t* pi = in + (uint64_t)u * 16;
    uint8_t* po = out + (uint64_t)u * 16;
    const uint32_t step = ustride * 16;   // rs_grid keeps a row of workgroups far below 4 GiB of blocks
    uint4 nc = aes_gload16(pi), np = aes_gload16(u ? pi - 16 : reinterpret_cast<const uint8_t*>(iv));
    for (;;) {
        const uint4 cblk = nc, prev = np;
        const bool more = nblk - u > ustride;   // no u + ustride: it may wrap
        if (more) {
            nc = aes_gload16(pi + step);
            np = aes_gload16(pi + step - 16);
        }
        uint4 x = aes_decrypt_block<NR>(cblk, dk, tab);
        x.x ^= prev.x;
        x.y ^= prev.y;
        x.z ^= prev.z;
        x.w ^= prev.w;
        if (u + 1 < nblk)
            aes_gstore16(po, x);
        else
            *pad_ok = (x.x == kAesPadWord && x.y == kAesPadWord && x.z == kAesPadWord && x.w == kAesPadWord) ? 1 : 0;
        if (!more) break;
        u += ustride;
        pi += step;
        po += step;
    }
}

constexpr int kAesDKeyedVWords = 12;

// Grid: x strides over a chain's blocks, y over chains (rs_grid), as aes_cbc_decrypt_kernel; every
// chain has nblk blocks (>= 2: the last one is the padding block; the host keeps nblk and nchain
// within 32 bits).  Descriptor and key entry depend on the chain alone: both tables are read-only
// for the launch and their addresses uniform over the workgroup, so they arrive by scalar loads,
// once per chain -- the key only when the chain's key index is not the previous chain's
// (rs_restore_kernel reloads its table on the same rule).  The round count is uniform too: one
// scalar branch per chain into the loop unrolled for it, so the round keys are indexed at compile
// time and stay in scalar registers.
__global__ __launch_bounds__(kAesDecThreads)
void aes_cbc_decrypt_keyed_kernel(const AesDChain* __restrict__ chains, const AesKeyEntry* __restrict__ keys,
                                  uint32_t nchain, uint32_t nblk, uint8_t* __restrict__ pad_ok) {
    __shared__ uint32_t tab[5 * 256];
    aes_fill_lds<kAesDecThreads>(tab, kAesTables.td0, kAesTables.inv);
    const uint32_t ustride = gridDim.x * kAesDecThreads;
    AesKey dk;
    uint32_t loaded = 0xffffffffu;   // no key's index
    for (uint32_t ch = blockIdx.y; ch < nchain; ch += gridDim.y) {
        const AesDChain d = chains[ch];
        const AesKeyEntry* k = keys + d.key;
        if (d.key != loaded) {
#pragma unroll
            for (int i = 0; i < dm_aes::kMaxKeyWords; i++) dk.w[i] = k->w[i];
            // 60 key words, three chain-invariant pointers and the loop's masks do not all fit the
            // scalar file: the first kAesDKeyedVWords words live in vector registers instead.  The
            // count is what this compiler needs to reach 0 spills (102 SGPRs); the guard is
            // tests/test_aes_dkeyed_codeobj.py, which fails on any spill or private segment.
#pragma unroll
            for (int i = 0; i < kAesDKeyedVWords; i++) asm("" : "+v"(dk.w[i]));
            loaded = d.key;
        }
        if (d.rounds == 10)
            aes_dkeyed_blocks<10>(d.in, d.out, nblk, ustride, dk, k->iv, tab, pad_ok + ch);
        else if (d.rounds == 12)
            aes_dkeyed_blocks<12>(d.in, d.out, nblk, ustride, dk, k->iv, tab, pad_ok + ch);
        else
            aes_dkeyed_blocks<14>(d.in, d.out, nblk, ustride, dk, k->iv, tab, pad_ok + ch);
    }
}

}  // namespace dm
