// rs_capi.inl -- Reed-Solomon fragment coding entry points (dm_rs_*, include/deoss_merkle.h).
// Part of merkle_capi.hip (included at its end; shares dm_ctx, Dev, DevBuf and the error helpers).
//
// Mirrors github.com/klauspost/reedsolomon v1.12.4 (go.mod:65) as the cess-go-sdk uses it for
// DeOSS fragments (New(chain.DataShards = 4, chain.ParShards = 8), node/tracker.go:250,369):
//   New(data, parity)      -> dm_rs_create   (default Vandermonde-derived systematic matrix), up to 8 + 8:
//                             the fragment coder every other dm_rs entry point takes;
//                             dm_rs_create_wide: klauspost's whole range, data + parity <= 256, for the
//                             calls listed here only (rs_code_wide_kernel beyond 8 + 8)
//   Encode(shards)         -> dm_rs_encode / dm_rs_encode_device_async
//   Reconstruct(shards)    -> dm_rs_reconstruct / dm_rs_reconstruct_device_async
//   Verify(shards)         -> dm_rs_verify
//   Split + Encode of one segment -> dm_rs_encode_buffer
// The GF(2^8) arithmetic (rs_plan.hpp) only builds the small coding tables; all shard bytes are coded
// by rs_code_kernel on the GPU (no CPU fallback).
#include "rs_kernels.hpp"   // includes rs_plan.hpp: the host side of the coding (matrices, tables, plans)
#include "rs_wide_kernels.hpp"

using namespace dm_rsplan;

namespace {

// One call lane's rs scratch: rs calls on different lanes of the first GPU run concurrently
// (dm_ctx call lanes), each with its own staging, so two uploads' FullProcessing overlap.
struct RsLane {
    DevBuf dec_tab;             // per reconstruct call
    DevBuf work;                // host-API shard staging, process parity, FullProcessing windows
    DevBuf rst_desc, rst_tab;   // restore, repair: per-segment descriptors, coding tables (restore_capi.inl, repair_capi.inl)
    PinnedBuf fp_slot[4];       // dm_full_processing: file / parity slots (fullproc_capi.inl)
};

}  // namespace

struct dm_rs {
    dm_ctx* c = nullptr;
    int k = 0, m = 0;
    bool wide = false;          // from dm_rs_create_wide beyond 8 + 8: rs_code_wide_kernel and its table layout
    std::vector<uint8_t> mat;   // (k + m) x k
    DevBuf enc_tab;             // parity rows, k x 256 x 8 B; wide: ceil(m / 8) x k x 32 x 8 B (read-only after the create call)
    std::vector<RsLane> ln;     // one per call lane of the context's first GPU
};

namespace {

// Lane of the context's first GPU (where an rs lives) for an rs call, counted in its load like
// pick_device (the caller's CallLock(..., kReserved) releases it).
int rs_lane(dm_ctx* c) {
    std::lock_guard<std::mutex> lk(c->route_mu);
    return choose_lane(c, 0, 0);
}

// The rs scratch of the lane d belongs to (d is one of r->c->devs, on the first GPU).
RsLane& rs_ln(dm_rs* r, const Dev& d) {
    return r->ln[(size_t)(&d - r->c->devs.data()) / (size_t)r->c->nphys];
}

// Grid of the rs kernels: x strides over a segment's 16-byte units, y over segments.
dim3 rs_grid(const Dev& d, uint64_t units, uint64_t nseg) {
    const uint64_t target = 8ull * (uint64_t)d.cus;   // workgroups in flight
    const uint32_t gy = (uint32_t)std::min<uint64_t>({nseg, 65535ull, target});
    const uint32_t gx = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(ceil_div(units, dm::kRsThreads),
                                                                           ceil_div(target, gy)));
    return dim3(gx, gy);
}

// f(std::integral_constant<int, K>()) for K = k: the rs kernels take the data shard count as a
// template argument (1 .. kRsMaxIn, checked by dm_rs_create).
template <class F>
void rs_for_k(int k, F&& f) {
    static_assert(dm::kRsMaxIn == 8, "one case per data shard count");
    switch (k) {
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 3: f(std::integral_constant<int, 3>()); break;
        case 4: f(std::integral_constant<int, 4>()); break;
        case 5: f(std::integral_constant<int, 5>()); break;
        case 6: f(std::integral_constant<int, 6>()); break;
        case 7: f(std::integral_constant<int, 7>()); break;
        default: f(std::integral_constant<int, 8>()); break;
    }
}

hipError_t launch_rs(Dev& d, hipStream_t s, int k, const dm::RsArgs& a) {
    const dim3 grid = rs_grid(d, a.units_per_seg, a.nseg), block(dm::kRsThreads);
    rs_for_k(k, [&](auto K) { hipLaunchKernelGGL(dm::rs_code_kernel<decltype(K)::value>, grid, block, 0, s, a); });
    return hipGetLastError();
}

// A wide coder's launch: rs_grid's x and y, one z layer per group of 8 outputs; nin x 256 B of LDS.
hipError_t launch_rs_wide(Dev& d, hipStream_t s, const dm::RsWideArgs& a) {
    dim3 grid = rs_grid(d, a.units_per_seg, a.nseg);
    grid.z = (a.nout + kRsGroup - 1) / kRsGroup;
    const size_t lds = (size_t)a.nin * kRsWideEntries * sizeof(uint2);
    hipLaunchKernelGGL(dm::rs_code_wide_kernel, grid, dim3(dm::kRsThreads), lds, s, a);
    return hipGetLastError();
}

// Every entry point outside the standalone coder's indexes kRsMaxIn / kRsMaxOut arrays by r->k and
// r->m: a wide coder is refused there before anything is allocated, opened or launched.
int rs_narrow(dm_rs* r, const char* fn) {
    if (!r->wide) return DM_OK;
    return fail(r->c, DM_ERR_INVALID, "%s needs a fragment coder of at most %d + %d shards", fn, dm::kRsMaxIn,
                dm::kRsMaxOut);
}

// Encode arguments for nseg segments: data shard j of segment t at data + t * data_stride +
// j * shard, parity shard i at parity + t * parity_stride + i * shard (r's parity rows).
dm::RsArgs rs_encode_args(const dm_rs* r, const uint8_t* data, uint64_t data_stride, uint8_t* parity,
                          uint64_t parity_stride, uint64_t shard, uint64_t nseg) {
    dm::RsArgs a{};
    for (int j = 0; j < r->k; j++) a.in[j] = data + (uint64_t)j * shard;
    for (int i = 0; i < r->m; i++) a.out[i] = parity + (uint64_t)i * shard;
    a.in_seg_stride = data_stride;
    a.out_seg_stride = parity_stride;
    a.units_per_seg = shard / 16;
    a.nseg = nseg;
    a.table = static_cast<const uint2*>(r->enc_tab.p);
    a.nout = (uint32_t)r->m;
    return a;
}

// Encode launch of either kind of coder, same layout as rs_encode_args.
hipError_t launch_rs_encode(dm_rs* r, Dev& d, hipStream_t s, const uint8_t* data, uint64_t data_stride, uint8_t* parity,
                            uint64_t parity_stride, uint64_t shard, uint64_t nseg) {
    if (!r->wide) return launch_rs(d, s, r->k, rs_encode_args(r, data, data_stride, parity, parity_stride, shard, nseg));
    dm::RsWideArgs a{};
    a.in_base = data;
    a.out_base = parity;
    a.in_pitch = a.out_pitch = shard;
    a.in_seg_stride = data_stride;
    a.out_seg_stride = parity_stride;
    a.units_per_seg = shard / 16;
    a.nseg = nseg;
    a.table = static_cast<const uint2*>(r->enc_tab.p);
    a.nin = (uint32_t)r->k;
    a.nout = (uint32_t)r->m;
    return launch_rs_wide(d, s, a);
}

// What rs_pick_inputs and the plans built on it return (rs_plan.hpp), as the call's error.
int plan_status(dm_ctx* c, int got, int k) {
    if (got == k) return DM_OK;
    if (got == kPlanSingular) return fail(c, DM_ERR_INVALID, "singular decode matrix");
    return fail(c, DM_ERR_INVALID, "too few shards given (%d of %d needed)", got, k);
}

// Rebuilds the missing shards from the first k present ones (klauspost Reconstruct; the plan is
// reconstruct_plan's, rs_plan.hpp) in one launch on s.
int rs_reconstruct_dev(dm_rs* r, Dev& d, hipStream_t s, uint8_t* const* shards, const uint8_t* present,
                       uint64_t pitch, uint64_t nbytes_units) {
    dm_ctx* c = r->c;
    ReconstructPlan p;
    RC_TRY(plan_status(c, reconstruct_plan(r->mat.data(), r->k, r->m, present, p), r->k));
    const int nmiss = (int)p.outputs.size();
    if (nmiss == 0) return DM_OK;
    RsLane& L = rs_ln(r, d);
    if (r->wide) {
        // the coding table, then the addresses of the k inputs and the nmiss outputs
        std::vector<uint64_t> tab = rs_wide_table(p.rows.data(), nmiss, r->k);
        const size_t ntab = tab.size();
        for (int j = 0; j < r->k; j++) tab.push_back((uint64_t)reinterpret_cast<uintptr_t>(shards[p.inputs[j]]));
        for (int t = 0; t < nmiss; t++) tab.push_back((uint64_t)reinterpret_cast<uintptr_t>(shards[p.outputs[t]]));
        RC_TRY(tables_begin(c, d, tab.size() * 8));
        RC_TRY(upload(c, d, s, L.dec_tab, tab.data(), tab.size() * 8));
        dm::RsWideArgs a{};
        a.addrs = static_cast<const uint64_t*>(L.dec_tab.p) + ntab;
        a.in_seg_stride = a.out_seg_stride = pitch;
        a.units_per_seg = nbytes_units;
        a.nseg = 1;
        a.table = static_cast<const uint2*>(L.dec_tab.p);
        a.nin = (uint32_t)r->k;
        a.nout = (uint32_t)nmiss;
        HIP_TRY(launch_rs_wide(d, s, a));
        return DM_OK;
    }
    const std::vector<uint64_t> tab = rs_table(p.rows.data(), nmiss, r->k);
    RC_TRY(tables_begin(c, d, tab.size() * 8));
    RC_TRY(upload(c, d, s, L.dec_tab, tab.data(), tab.size() * 8));
    dm::RsArgs a{};
    for (int j = 0; j < r->k; j++) a.in[j] = shards[p.inputs[j]];
    for (int t = 0; t < nmiss; t++) a.out[t] = shards[p.outputs[t]];
    a.in_seg_stride = a.out_seg_stride = pitch;
    a.units_per_seg = nbytes_units;
    a.nseg = 1;
    a.table = static_cast<const uint2*>(L.dec_tab.p);
    a.nout = (uint32_t)nmiss;
    HIP_TRY(launch_rs(d, s, r->k, a));
    return DM_OK;
}

// The coder of k + m shards on ctx's first GPU (counts checked by the caller, who holds the lock).
int rs_create(dm_ctx* ctx, int k, int m, bool wide, dm_rs** out) {
    dm_ctx* c = ctx;
    dm_rs* r = new (std::nothrow) dm_rs();
    if (!r) return fail(c, DM_ERR_NOMEM, "dm_rs_create: out of host memory");
    r->c = ctx;
    r->k = k;
    r->m = m;
    r->wide = wide;
    if (!(wide ? rs_build_matrix_n(k, m, r->mat) : rs_build_matrix(k, m, r->mat))) {
        delete r;
        return fail(c, DM_ERR_INVALID, "singular Vandermonde top");
    }
    const uint8_t* prows = r->mat.data() + (size_t)k * k;
    const std::vector<uint64_t> tab = wide ? rs_wide_table(prows, m, k) : rs_table(prows, m, k);
    Dev& d = ctx->devs[0];
    r->ln.resize((size_t)ctx->lanes);
    r->enc_tab.rp = &ctx->reaper;
    r->enc_tab.dev = d.id;
    for (RsLane& L : r->ln)
        for (DevBuf* b : {&L.dec_tab, &L.work, &L.rst_desc, &L.rst_tab}) {
            b->rp = &ctx->reaper;   // growth (work: FullProcessing windows) never synchronises the device
            b->dev = d.id;
        }
    hipError_t e = hipSetDevice(d.id);
    if (e == hipSuccess) e = r->enc_tab.ensure(tab.size() * 8);
    // on the first lane's copy stream (non-blocking), not hipMemcpy's null stream: that one would
    // wait for every lane's queued chains on this GPU (their compute streams order with it)
    if (e == hipSuccess) e = hipMemcpyAsync(r->enc_tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, d.copy);
    if (e == hipSuccess) e = hipStreamSynchronize(d.copy);
    if (e != hipSuccess) {
        r->enc_tab.release();
        delete r;
        return fail(c, DM_ERR_HIP, "dm_rs_create: %s", hipGetErrorString(e));
    }
    *out = r;
    return DM_OK;
}

// klauspost's New: ErrInvShardNum, ErrMaxShardNum (a coder without parity codes nothing here).
int rs_wide_counts(dm_ctx* c, int data, int parity) {
    if (data < 1)
        return fail(c, DM_ERR_INVALID,
                    "cannot create Encoder with less than one data shard or less than zero parity shards");
    if (parity < 1) return fail(c, DM_ERR_INVALID, "cannot create Encoder with less than one parity shard");
    if (data + parity > kRsWideMaxShards)
        return fail(c, DM_ERR_INVALID, "cannot create Encoder with more than 256 data+parity shards");
    return DM_OK;
}

}  // namespace

extern "C" {

int dm_rs_create(dm_ctx* ctx, int data_shards, int parity_shards, dm_rs** out) {
    if (!ctx || !out) return bad_arg();
    *out = nullptr;
    CallLock lk(ctx, 0);
    dm_ctx* c = ctx;
    if (data_shards < 1 || data_shards > dm::kRsMaxIn || parity_shards < 1 || parity_shards > dm::kRsMaxOut)
        return fail(c, DM_ERR_INVALID, "shard counts: 1 <= data <= %d, 1 <= parity <= %d", dm::kRsMaxIn,
                    dm::kRsMaxOut);
    return rs_create(ctx, data_shards, parity_shards, false, out);
}

int dm_rs_create_wide(dm_ctx* ctx, int data_shards, int parity_shards, dm_rs** out) {
    if (!ctx || !out) return bad_arg();
    *out = nullptr;
    CallLock lk(ctx, 0);
    RC_TRY(rs_wide_counts(ctx, data_shards, parity_shards));
    // DEOSS_RS_FORCE_WIDE (measurement only, tools/rs_wide_ab.py): the wide kernel within 8 + 8 too
    static const bool force = std::getenv("DEOSS_RS_FORCE_WIDE") != nullptr;
    const bool wide = data_shards > dm::kRsMaxIn || parity_shards > dm::kRsMaxOut || force;
    return rs_create(ctx, data_shards, parity_shards, wide, out);
}

int dm_rs_coding_matrix(int data, int parity, uint8_t* out) {
    if (!out) return bad_arg();
    RC_TRY(rs_wide_counts(nullptr, data, parity));
    std::vector<uint8_t> mat;
    if (!rs_build_matrix_n(data, parity, mat)) return fail(nullptr, DM_ERR_INVALID, "singular Vandermonde top");
    std::memcpy(out, mat.data(), mat.size());
    return DM_OK;
}

void dm_rs_destroy(dm_rs* r) {
    if (!r) return;
    {
        RangeLock lk(r->c);   // after every call in flight on any lane
        (void)hipSetDevice(r->c->devs[0].id);
        (void)hipDeviceSynchronize();
        r->enc_tab.release();
        for (RsLane& L : r->ln) {
            L.dec_tab.release();
            L.work.release();
            L.rst_desc.release();
            L.rst_tab.release();
            for (auto& b : L.fp_slot) b.release();
        }
    }
    delete r;
}

int dm_rs_matrix(dm_rs* r, uint8_t* out) {
    if (!r || !out) return bad_arg();
    std::memcpy(out, r->mat.data(), r->mat.size());
    return DM_OK;
}

int dm_rs_encode_device_async(dm_rs* r, const void* data, uint64_t data_stride, void* parity, uint64_t parity_stride,
                              uint64_t shard, uint64_t nseg, void* stream) {
    if (!r) return bad_arg();
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    if (!data || !parity || nseg == 0 || shard == 0 || shard % 16 || data_stride % 16 || parity_stride % 16 ||
        !is_aligned16(data) || !is_aligned16(parity))
        return fail(c, DM_ERR_INVALID, "dm_rs_encode_device_async: need 16-byte aligned shards, strides and sizes");
    Dev& d = c->devs[g];
    hipStream_t s = pick_stream(d, stream);
    RC_TRY(begin_call(c, d, s));
    hipEvent_t* tr = timing_record(c, d);
    if (tr) HIP_TRY(hipEventRecord(tr[0], s));
    HIP_TRY(launch_rs_encode(r, d, s, static_cast<const uint8_t*>(data), data_stride, static_cast<uint8_t*>(parity),
                             parity_stride, shard, nseg));
    if (tr) {
        HIP_TRY(hipEventRecord(tr[1], s));
        HIP_TRY(hipEventRecord(tr[2], s));
    }
    return DM_OK;
}

int dm_rs_reconstruct_device_async(dm_rs* r, void* const* shards, const uint8_t* present, uint64_t shard,
                                   void* stream) {
    if (!r) return bad_arg();
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    if (!shards || !present || shard == 0 || shard % 16)
        return fail(c, DM_ERR_INVALID, "dm_rs_reconstruct_device_async: shard bytes must be a multiple of 16");
    for (int i = 0; i < r->k + r->m; i++)
        if (!shards[i] || !is_aligned16(shards[i]))
            return fail(c, DM_ERR_INVALID, "dm_rs_reconstruct_device_async: shard %d null or not 16-byte aligned", i);
    Dev& d = c->devs[g];
    hipStream_t s = pick_stream(d, stream);
    RC_TRY(begin_call(c, d, s));
    return rs_reconstruct_dev(r, d, s, reinterpret_cast<uint8_t* const*>(shards), present, shard, shard / 16);
}

// Host shards: staged in one device buffer at a 16-byte pitch (padding positions are coded too
// and never copied back; positions are independent).
int dm_rs_encode(dm_rs* r, const void* const* data, void* const* parity, uint64_t shard) {
    if (!r) return bad_arg();
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    if (!data || !parity || shard == 0) return fail(c, DM_ERR_INVALID, "dm_rs_encode: null shards or zero size");
    for (int j = 0; j < r->k; j++)
        if (!data[j]) return fail(c, DM_ERR_INVALID, "dm_rs_encode: data shard %d is null", j);
    for (int i = 0; i < r->m; i++)
        if (!parity[i]) return fail(c, DM_ERR_INVALID, "dm_rs_encode: parity shard %d is null", i);
    Dev& d = c->devs[g];
    DevBuf& work = rs_ln(r, d).work;
    hipStream_t s = d.stream;
    RC_TRY(begin_call(c, d, s));
    const uint64_t pitch = round_up(shard, 16);
    const int total = r->k + r->m;
    HIP_TRY(work.ensure(pitch * total));
    for (int j = 0; j < r->k; j++)
        HIP_TRY(hipMemcpyAsync(work.u8() + j * pitch, data[j], shard, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_rs_encode(r, d, s, work.u8(), 0, work.u8() + r->k * pitch, 0, pitch, 1));
    for (int i = 0; i < r->m; i++)
        HIP_TRY(hipMemcpyAsync(parity[i], work.u8() + (r->k + i) * pitch, shard, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return DM_OK;
}

int dm_rs_encode_buffer(dm_rs* r, const void* host, uint64_t len, void* out, uint64_t* per_shard) {
    if (!r) return bad_arg();
    if (!per_shard || !out || (!host && len)) return fail(r->c, DM_ERR_INVALID, "dm_rs_encode_buffer: null argument");
    if (len == 0) return fail(r->c, DM_ERR_EMPTY, "Empty data");   // klauspost ErrShortData
    const uint64_t per = ceil_div(len, (uint64_t)r->k);
    *per_shard = per;
    uint8_t* o = static_cast<uint8_t*>(out);
    // Split: data shards are the buffer in order, the last one zero-padded
    std::memcpy(o, host, len);
    std::memset(o + len, 0, per * r->k - len);
    std::vector<const void*> dp(r->k);
    std::vector<void*> pp(r->m);
    for (int j = 0; j < r->k; j++) dp[j] = o + j * per;
    for (int i = 0; i < r->m; i++) pp[i] = o + (r->k + i) * per;
    return dm_rs_encode(r, dp.data(), pp.data(), per);
}

int dm_rs_reconstruct(dm_rs* r, void* const* shards, const uint8_t* present, uint64_t shard) {
    if (!r) return bad_arg();
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    const int total = r->k + r->m;
    if (!shards || !present || shard == 0) return fail(c, DM_ERR_INVALID, "dm_rs_reconstruct: bad arguments");
    for (int i = 0; i < total; i++)
        if (!shards[i]) return fail(c, DM_ERR_INVALID, "dm_rs_reconstruct: shard %d is null", i);
    int nv = 0;
    for (int i = 0; i < total; i++) nv += present[i] != 0;
    if (nv == total) return DM_OK;
    if (nv < r->k) return plan_status(c, nv, r->k);
    Dev& d = c->devs[g];
    DevBuf& work = rs_ln(r, d).work;
    hipStream_t s = d.stream;
    RC_TRY(begin_call(c, d, s));
    const uint64_t pitch = round_up(shard, 16);
    HIP_TRY(work.ensure(pitch * total));
    std::vector<uint8_t*> dev(total);
    for (int i = 0; i < total; i++) {
        dev[i] = work.u8() + i * pitch;
        if (present[i]) HIP_TRY(hipMemcpyAsync(dev[i], shards[i], shard, hipMemcpyHostToDevice, s));
    }
    RC_TRY(rs_reconstruct_dev(r, d, s, dev.data(), present, pitch, pitch / 16));
    for (int i = 0; i < total; i++)
        if (!present[i]) HIP_TRY(hipMemcpyAsync(shards[i], dev[i], shard, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return DM_OK;
}

int dm_rs_verify(dm_rs* r, const void* const* shards, uint64_t shard, int* ok) {
    if (!r || !ok) return bad_arg();
    *ok = 0;
    if (!shards || shard == 0) return fail(r->c, DM_ERR_INVALID, "dm_rs_verify: bad arguments");
    std::vector<std::vector<uint8_t>> mine(r->m, std::vector<uint8_t>(shard));
    std::vector<void*> pp(r->m);
    for (int i = 0; i < r->m; i++) pp[i] = mine[i].data();
    RC_TRY(dm_rs_encode(r, shards, pp.data(), shard));
    for (int i = 0; i < r->m; i++) {
        if (!shards[r->k + i]) return fail(r->c, DM_ERR_INVALID, "dm_rs_verify: parity shard %d is null", i);
        if (std::memcmp(mine[i].data(), shards[r->k + i], shard) != 0) return DM_OK;
    }
    *ok = 1;
    return DM_OK;
}

}  // extern "C"
