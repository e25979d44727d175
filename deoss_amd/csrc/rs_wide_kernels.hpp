// rs_wide_kernels.hpp -- gfx950 Reed-Solomon coding for any geometry up to 256 shards
// (dm_rs_create_wide).  Included by rs_capi.inl only, after rs_kernels.hpp, whose kernels it leaves
// as they are: geometries within 8 + 8 never come here.
//
// out[i] = sum_j M[i][j] * in[j] over GF(2^8) for a run-time nin <= 255 and nout <= 255.  The
// outputs go in groups of 8: as in rs_code_kernel one 8-byte table entry carries a byte's
// contribution to 8 outputs at the same position, a lane owns 16 consecutive positions and keeps
// their 16 accumulators in registers, and the position-major accumulators become shard-major words
// by rs_kernels.hpp's rs_shard_words.  What differs from its rs_code_units:
//   - the inputs are walked by a run-time loop (one 16-B load in flight while the previous input is
//     looked up), so every output group reads all nin inputs again: per segment nin * ceil(nout/8)
//     shard reads and nout shard writes, no read-modify-write of partial outputs;
//   - the table is split by nibble, x * c = (x & 15) * c ^ (x & 0xf0) * c: per input 16 + 16
//     entries of 8 B = 256 B of LDS (rs_plan.hpp: rs_wide_table), 65,280 B at 255 inputs, against
//     2 KiB per input for a byte table.  One ds_read_b64 reads one input's low or high table: 16
//     distinct entries in one aligned 128-B half of an LDS bank row (bank = (addr / 4) % 64), each on
//     two banks of its own, so whatever bytes the lanes hold the read has no bank conflict;
//   - shard addresses are base + index * pitch (encode) or come from a device table of nin + nout
//     addresses (reconstruct); the index is the same in every lane, so those loads are wave-uniform.
#pragma once
#include "rs_kernels.hpp"

namespace dm {

using dm_rsplan::kRsGroup;         // 8 outputs per table entry
using dm_rsplan::kRsWideEntries;   // 32 table entries per input and group (rs_plan.hpp: rs_wide_table)

struct RsWideArgs {
    const uint8_t* in_base;        // addrs == nullptr: input j of segment 0 at in_base + j * in_pitch
    uint8_t* out_base;             //                   output i of segment 0 at out_base + i * out_pitch
    uint64_t in_pitch;
    uint64_t out_pitch;
    const uint64_t* addrs;         // else [nin + nout] device addresses: the inputs, then the outputs
    uint64_t in_seg_stride;        // bytes from segment s to s+1 (inputs)
    uint64_t out_seg_stride;       // bytes from segment s to s+1 (outputs)
    uint64_t units_per_seg;        // shard bytes / 16
    uint64_t nseg;
    const uint2* table;            // [ceil(nout / 8)][nin][32] x 8 B
    uint32_t nin;
    uint32_t nout;
};

// Shard addresses are integers here: one from the address table is no kernel argument, so the
// compiler cannot tell that it points to global memory; the loads and stores below say so.
typedef const __attribute__((address_space(1))) rs_u32x4* rs_gload_t;
typedef __attribute__((address_space(1))) rs_u32x4* rs_gstore_t;
// the address table is read-only for the whole launch: constant address space, scalar loads
typedef const __attribute__((address_space(4))) uint64_t* rs_addr_table_t;

__device__ __forceinline__ uint64_t rs_wide_in(const RsWideArgs& a, uint32_t j) {
    return a.addrs ? reinterpret_cast<rs_addr_table_t>(reinterpret_cast<uintptr_t>(a.addrs))[j]
                   : reinterpret_cast<uintptr_t>(a.in_base) + (uint64_t)j * a.in_pitch;
}

__device__ __forceinline__ uint64_t rs_wide_out(const RsWideArgs& a, uint32_t i) {
    return a.addrs ? reinterpret_cast<rs_addr_table_t>(reinterpret_cast<uintptr_t>(a.addrs))[a.nin + i]
                   : reinterpret_cast<uintptr_t>(a.out_base) + (uint64_t)i * a.out_pitch;
}

__device__ __forceinline__ uint4 rs_wide_load(uint64_t addr) {
    const rs_u32x4 v = *reinterpret_cast<rs_gload_t>(addr);
    return make_uint4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ void rs_wide_store(uint64_t addr, uint4 v) {
    const rs_u32x4 w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<rs_gstore_t>(addr));
}

// Grid: x strides over a segment's 16-byte units, y over segments, z over the output groups.
// Dynamic LDS: nin * 256 bytes.  The group, like the segment, depends on the block index alone, so
// every wave of a workgroup meets the same barriers.
__global__ __launch_bounds__(kRsThreads)
void rs_code_wide_kernel(RsWideArgs a) {
    extern __shared__ uint2 rs_wide_tab[];
    const uint32_t nent = a.nin * kRsWideEntries;
    const uint32_t groups = (a.nout + kRsGroup - 1) / kRsGroup;
    const uint64_t ustride = (uint64_t)gridDim.x * kRsThreads;
    for (uint32_t g = blockIdx.z; g < groups; g += gridDim.z) {
        if (g != blockIdx.z) __syncthreads();   // every wave is done with the previous group's table
        const uint2* src = a.table + (uint64_t)g * nent;
        for (uint32_t t = threadIdx.x; t < nent; t += kRsThreads) rs_wide_tab[t] = src[t];
        __syncthreads();
        const uint32_t o0 = g * kRsGroup;
        const uint32_t no = min(a.nout - o0, (uint32_t)kRsGroup);   // outputs of this group: 1..8
        for (uint64_t seg = blockIdx.y; seg < a.nseg; seg += gridDim.y) {
            const uint64_t ib = seg * a.in_seg_stride;
            const uint64_t ob = seg * a.out_seg_stride;
            for (uint64_t u = (uint64_t)blockIdx.x * kRsThreads + threadIdx.x; u < a.units_per_seg; u += ustride) {
                const uint64_t off = u * 16;
                uint2 acc[16];
#pragma unroll
                for (int p = 0; p < 16; p++) acc[p] = make_uint2(0, 0);
                uint4 nx = rs_wide_load(rs_wide_in(a, 0) + ib + off);
                for (uint32_t j = 0; j < a.nin; j++) {
                    const uint4 x = nx;
                    // the next input's load is in flight while this one is looked up
                    if (j + 1 < a.nin) nx = rs_wide_load(rs_wide_in(a, j + 1) + ib + off);
                    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
                    const uint2* tj = rs_wide_tab + j * kRsWideEntries;
#pragma unroll
                    for (int q = 0; q < 4; q++) {
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const uint32_t b = (w[q] >> (8 * k)) & 0xffu;
                            const uint2 lo = tj[b & 15u];
                            const uint2 hi = tj[16u + (b >> 4)];
                            acc[4 * q + k].x ^= lo.x ^ hi.x;
                            acc[4 * q + k].y ^= lo.y ^ hi.y;
                        }
                    }
                }
                // output o0 + i, word q = byte i of acc[4q .. 4q+3]
                uint32_t lo[4][4], hi[4][4];   // [q][row]
                rs_shard_words<true>(acc, lo, hi);
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i < (int)no)
                        rs_wide_store(rs_wide_out(a, o0 + i) + ob + off,
                                      make_uint4(lo[0][i], lo[1][i], lo[2][i], lo[3][i]));
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i + 4 < (int)no)
                        rs_wide_store(rs_wide_out(a, o0 + i + 4) + ob + off,
                                      make_uint4(hi[0][i], hi[1][i], hi[2][i], hi[3][i]));
            }
        }
    }
}

}  // namespace dm
