// range_capi.inl -- ranged restore on the GPU: bytes [off, off + len) of an object from just the
// fragments that cover them (dm_range_plan, dm_restore_range_buffer, dm_retrieve_range;
// include/deoss_merkle.h).  Part of merkle_capi.hip (after repair_capi.inl; shares rt_hash, rt_load,
// RtStatus, rs_desc_launch and the pinned slots with the restore and repair paths).  The plan is
// range_plan.hpp, the window decryption aes_cbc_decrypt_window_kernel (cipher_capi.inl).
//
// Replaces, for the HTTP Range of GET /file/open (node/fileHandler.go:399-545), the whole-object
// process.Retrievefile that precedes ReturnFileRangeStream on a cache miss.  Per call (or per window
// of touched segments), in rounds as in repair_capi.inl:
//   1. of every touched segment the needed data fragments go to HBM, each at its final place in a
//      segment-strided buffer; where one of them is missing or known bad, the first k usable
//      fragments in index order instead (parity to scratch);
//   2. (DM_RESTORE_VERIFY_FRAGMENTS) ONE table-mode leaf launch hashes what was brought; a fragment
//      that is not its name is bad, and absent in the next round;
//   3. ONE repair launch rebuilds the needed data fragments that are not usable (no other), ONE leaf
//      launch checks them against their names: a rebuilt fragment proves itself;
//   4. with a cipher ONE window launch decrypts the range's blocks and checks the paddings the plan
//      names;
//   5. the bytes leave the device only when every touched segment is ok.
// Segment names and the fid are not checked: they are names of whole segments, which a ranged
// restore never has.  The cipher scheme is RECALLED, NOT PINNED (cipher_scheme.hpp).
#include "range_plan.hpp"

namespace {

// One ranged call: the plan and the whole-object arrays it reports into.
struct RangeCall {
    dm_rs* r;
    Dev* d;
    dm_range::Plan plan;
    uint64_t segment, off, len;
    const uint8_t* names;    // whole object; null: fragments are used as given
    const CipherKey* key;    // null: no cipher
    uint8_t* fst;            // whole object
    uint8_t* sst;
};

// Brings fragments of a run of touched segments to the device (idx = t * total + j within the run);
// complete, or queued on the compute stream, on return.
using RangeLoad = std::function<int(const std::vector<RtLoad>&)>;

// Steps 1 - 4 for touched segments [t0, t0 + ns).  given[t * total + j]: there is a fragment to load
// (it may still be bad).  *good: every segment of the run is ok, and the run's bytes of the range,
// *nbytes of them, lie at *src on the device (valid until the lane's next launch).
int range_run(RangeCall& q, uint64_t t0, uint64_t ns, const std::vector<uint8_t>& given, const RangeLoad& load, bool* good,
              const uint8_t** src, uint64_t* nbytes) {
    dm_rs* r = q.r;
    dm_ctx* c = r->c;
    Dev& d = *q.d;
    hipStream_t s = d.stream;
    RsLane& L = rs_ln(r, d);
    const int k = r->k, m = r->m, total = r->k + r->m;
    const uint64_t segment = q.segment, frag = segment / (uint64_t)k, s0 = q.plan.seg0 + t0;
    const uint64_t piece = q.key ? segment - dm_cipher::kBlock : segment;
    *good = false;
    // the run's windows, and where its plaintext goes (joined position s * P + 16 * b0 keeps 16-byte
    // alignment: everything is placed relative to pos0, a multiple of 16)
    size_t w0 = 0, w1 = 0;
    while (w0 < q.plan.win.size() && q.plan.win[w0].seg < s0) w0++;
    for (w1 = w0; w1 < q.plan.win.size() && q.plan.win[w1].seg < s0 + ns; w1++) {}
    const uint64_t nwin = w1 - w0;
    const uint64_t beg = std::max(q.off, s0 * piece), end = std::min(q.off + q.len, (s0 + ns) * piece);
    const uint64_t pos0 = beg / 16 * 16, plain_len = round_up(end - pos0, 16);
    uint64_t npar = 0;
    for (uint64_t t = 0; t < ns; t++)
        for (int j = k; j < total; j++) npar += given[t * total + j] != 0;
    HIP_TRY(hipStreamSynchronize(s));   // the previous run's kernels are done with the buffers
    HIP_TRY(d.data.ensure(ns * segment + kAlign));
    // scratch: parity inputs | plaintext | one dump block per window | one verdict per window
    const uint64_t plain_off = round_up(npar * frag + 16, kAlign), dump_off = plain_off + plain_len;
    HIP_TRY(L.work.ensure(q.key ? dump_off + 16 * nwin + nwin : npar * frag + 16));
    uint8_t* base = d.data.u8();

    enum : uint8_t { kNone, kGiven, kGood, kBad };
    const uint64_t NF = ns * (uint64_t)total;
    std::vector<uint8_t> st(NF, kNone), active(ns, 1), used(NF, 0), rebuilt(NF, 0);
    std::vector<uint8_t*> slot(NF, nullptr);
    for (uint64_t i = 0; i < NF; i++)
        if (given[i]) st[i] = kGiven;
    auto usable = [&](uint64_t i) { return st[i] == kGiven || st[i] == kGood; };
    uint8_t* wf = q.fst + s0 * total;
    uint8_t* ws = q.sst + s0;
    const uint8_t* need0 = q.plan.need.data() + t0 * (uint64_t)k;
    const uint8_t* wnames = q.names ? q.names + 32 * s0 * total : nullptr;
    uint64_t bump = 0, nactive = ns;
    struct Seg {
        uint64_t t;
        int sel[dm::kRsMaxIn], nsel;
        bool direct;
    };
    for (int round = 0; nactive > 0; round++) {
        // 1. per segment the needed data fragments, or the first k usable ones
        std::vector<Seg> segs;
        std::vector<RtLoad> loads;
        for (uint64_t t = 0; t < ns; t++) {
            if (!active[t]) continue;
            const uint64_t f0 = t * total;
            Seg sg{};
            sg.t = t;
            sg.direct = true;
            for (int j = 0; j < k; j++)
                if (need0[t * k + j] && !usable(f0 + j)) sg.direct = false;
            for (int j = 0; j < total && sg.nsel < k; j++)
                if (sg.direct ? (j < k && need0[t * k + j]) : usable(f0 + j)) sg.sel[sg.nsel++] = j;
            if (!sg.direct && sg.nsel < k) {
                ws[t] = kSegTooFew;
                active[t] = 0;
                nactive--;
                continue;
            }
            for (int e = 0; e < sg.nsel; e++) {
                const int j = sg.sel[e];
                const uint64_t i = f0 + j;
                if (st[i] != kGiven || slot[i]) continue;
                slot[i] = j < k ? base + t * segment + (uint64_t)j * frag : L.work.u8() + (bump++) * frag;
                loads.push_back({i, slot[i]});
            }
            segs.push_back(sg);
        }
        if (segs.empty()) break;
        if (round > m) return fail(c, DM_ERR_INVALID, "ranged restore: more than parity + 1 rounds");   // every other round condemns a fragment
        RC_TRY(load(loads));
        hipEvent_t* tr = timing_record(c, d);   // one record per round
        if (tr) HIP_TRY(hipEventRecord(tr[0], s));
        // 2. what was brought against its names
        std::vector<uint8_t> dig;
        if (wnames) {
            std::vector<uint64_t> addrs;
            for (const RtLoad& l : loads) addrs.push_back(reinterpret_cast<uint64_t>(l.to));
            RC_TRY(rt_hash(c, d, s, addrs, frag, dig));
        }
        for (size_t e = 0; e < loads.size(); e++) {
            const uint64_t i = loads[e].idx;
            const bool ok = !wnames || std::memcmp(dig.data() + 32 * e, wnames + 32 * i, 32) == 0;
            st[i] = ok ? kGood : kBad;
            if (!ok) wf[i] = kFragBad;
        }
        // 3. one repair launch for every segment that rebuilds anything, its outputs against their names
        RepairBatch b{r->mat.data(), k, m};
        std::vector<std::pair<uint64_t, uint8_t*>> outs;   // fragment, where it is rebuilt
        std::vector<const Seg*> settled;
        for (const Seg& sg : segs) {
            const uint64_t t = sg.t, f0 = t * total;
            bool bad_in = false;
            for (int e = 0; e < sg.nsel; e++) bad_in |= st[f0 + sg.sel[e]] == kBad;
            if (bad_in) continue;   // the next round chooses again
            settled.push_back(&sg);
            if (sg.direct) continue;
            uint8_t* ptr[dm::kRsMaxIn + dm::kRsMaxOut] = {};
            uint8_t present[dm::kRsMaxIn + dm::kRsMaxOut] = {};
            for (int e = 0; e < sg.nsel; e++) {
                ptr[sg.sel[e]] = slot[f0 + sg.sel[e]];
                present[sg.sel[e]] = 1;
            }
            for (int j = 0; j < k; j++)
                if (need0[t * k + j] && !usable(f0 + j)) {
                    ptr[j] = base + t * segment + (uint64_t)j * frag;
                    outs.emplace_back(f0 + j, ptr[j]);
                }
            RC_TRY(plan_status(c, repair_add(b, ptr, present), k));
        }
        RC_TRY(rs_desc_launch(r, d, s, b, frag / 16));
        dig.clear();
        if (wnames && !outs.empty()) {
            std::vector<uint64_t> addrs;
            for (const auto& o : outs) addrs.push_back(reinterpret_cast<uint64_t>(o.second));
            RC_TRY(rt_hash(c, d, s, addrs, frag, dig));
        }
        if (tr) {
            HIP_TRY(hipEventRecord(tr[1], s));
            HIP_TRY(hipEventRecord(tr[2], s));
        }
        for (size_t e = 0; e < outs.size(); e++) {
            const uint64_t i = outs[e].first;
            if (wnames && std::memcmp(dig.data() + 32 * e, wnames + 32 * i, 32) != 0) {
                ws[i / total] = kSegMismatch;   // good inputs, another output: the names do not belong together
                continue;
            }
            st[i] = kGood;
            slot[i] = outs[e].second;
            if (wf[i] != kFragBad) wf[i] = kFragRebuilt;   // a given fragment that was bad stays reported as bad
            rebuilt[i] = 1;
        }
        for (const Seg* sg : settled) {
            for (int e = 0; e < sg->nsel; e++) used[sg->t * total + sg->sel[e]] = 1;
            active[sg->t] = 0;
            nactive--;
        }
    }
    bool all = true;
    for (uint64_t i = 0; i < NF; i++)
        if (st[i] == kGood && !rebuilt[i]) wf[i] = used[i] ? kFragUsed : kFragSpare;
    for (uint64_t t = 0; t < ns; t++) all &= ws[t] == kSegOk;
    if (!all) return DM_OK;
    if (!q.key) {   // a plain device range: no kernel runs
        *src = base + (beg - s0 * piece);
        *nbytes = end - beg;
        *good = true;
        return DM_OK;
    }
    // 4. one window launch; a window of the last two blocks decrypts into a dump block
    uint8_t* plain = L.work.u8() + plain_off;
    uint8_t* dump = L.work.u8() + dump_off;
    uint8_t* pad_ok = dump + 16 * nwin;
    std::vector<dm::AesWindow> win(nwin);
    for (uint64_t w = 0; w < nwin; w++) {
        const dm_range::Window& x = q.plan.win[w0 + w];
        const uint8_t* in = base + (x.seg - s0) * segment + x.first;
        dm::AesWindow& a = win[w];
        a.in = in;
        a.nblk = x.bytes / 16;
        a.check_pad = (x.flags & dm_range::kWinCheckPad) ? 1 : 0;
        if (x.flags & dm_range::kWinPadOnly) {
            a.prev = in;   // its first block's plaintext is dumped: any loaded block will do
            a.out = dump + 16 * w;
        } else {
            a.prev = (x.flags & dm_range::kWinPrevIv) ? nullptr : in - 16;
            a.out = plain + (x.seg * piece + x.first - pos0);
        }
    }
    RC_TRY(launch_aes_decrypt_windows(c, d, s, *q.key, win, pad_ok));
    std::vector<uint8_t> pad(nwin);
    HIP_TRY(hipMemcpyAsync(pad.data(), pad_ok, nwin, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint64_t w = 0; w < nwin; w++)
        if (win[w].check_pad && pad[w] != 1) {
            ws[q.plan.win[w0 + w].seg - s0] = kSegBadPadding;
            all = false;
        }
    if (!all) return DM_OK;
    *src = plain + (beg - pos0);
    *nbytes = end - beg;
    *good = true;
    return DM_OK;
}

// The arguments both ranged entry points share: the restore's, then the plan.
int range_check(dm_rs* r, uint64_t nseg, uint64_t size, uint64_t segment, uint64_t off, uint64_t len, int flags,
                CipherKey* key, const void* cipher, uint64_t cipher_len, dm_range::Plan& plan) {
    dm_ctx* c = r->c;
    RC_TRY(restore_check(r, nseg, size, segment, key, cipher, cipher_len));
    const std::string err = dm_range::plan(size, nseg, segment, r->k, key != nullptr, off, len, flags, plan);
    if (!err.empty()) return fail(c, DM_ERR_INVALID, "%s", err.c_str());
    return DM_OK;
}

// Touched segments in runs of `win`: a range within one run leaves the device only after every check;
// a longer one is staged in pageable host memory and copied to `out` at the end, so nothing is
// written unless all is good and neither device nor pinned memory grows with len.
template <class Given>
int range_windows(RangeCall& q, uint64_t win, Given&& given_of, const RangeLoad& load, void* out, int* ok) {
    Dev& d = *q.d;
    dm_ctx* c = q.r->c;
    hipStream_t s = d.stream;
    const uint64_t nt = q.plan.ntouched;
    const bool one = nt <= win;
    std::vector<uint8_t> staged(one ? 0 : q.len);
    bool all = true;
    uint64_t done = 0;
    for (uint64_t t0 = 0; t0 < nt; t0 += win) {
        const uint64_t ns = std::min(win, nt - t0);
        std::vector<uint8_t> given;
        RC_TRY(given_of(t0, ns, given));
        bool good = false;
        const uint8_t* src = nullptr;
        uint64_t nbytes = 0;
        RC_TRY(range_run(q, t0, ns, given, load, &good, &src, &nbytes));
        if (!good) all = false;   // later runs still report their fragments
        if (!all) continue;
        HIP_TRY(hipMemcpyAsync(one ? out : staged.data() + done, src, nbytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        done += nbytes;
    }
    if (all && !one) std::memcpy(out, staged.data(), q.len);
    *ok = all ? 1 : 0;
    return DM_OK;
}

}  // namespace

extern "C" {

int dm_range_plan(uint64_t size, uint64_t nseg, uint64_t segment, int data, int cipher, uint64_t off, uint64_t len,
                  int flags, uint64_t* seg0, uint64_t* ntouched, uint8_t* need, uint64_t need_cap, dm_range_window* windows,
                  uint64_t win_cap, uint64_t* nwin) {
    if (!seg0 || !ntouched || !nwin) return bad_arg();
    dm_range::Plan p;
    const std::string err = dm_range::plan(size, nseg, segment, data, cipher != 0, off, len, flags, p);
    if (!err.empty()) return fail(nullptr, DM_ERR_INVALID, "%s", err.c_str());
    *seg0 = p.seg0;
    *ntouched = p.ntouched;
    *nwin = p.win.size();
    if ((need && need_cap < p.need.size()) || (windows && win_cap < p.win.size()))
        return fail(nullptr, DM_ERR_INVALID, "dm_range_plan: %llu segments and %llu windows do not fit the arrays given",
                    (unsigned long long)p.ntouched, (unsigned long long)p.win.size());
    if (need) std::memcpy(need, p.need.data(), p.need.size());
    if (windows)
        for (size_t w = 0; w < p.win.size(); w++)
            windows[w] = dm_range_window{p.win[w].seg, p.win[w].first, p.win[w].bytes, p.win[w].flags, 0};
    return DM_OK;
}

int dm_restore_range_buffer(dm_rs* r, const void* const* frags, const uint8_t* frag_names, uint64_t nseg, uint64_t size,
                            uint64_t segment, uint64_t off, uint64_t len, int flags, const void* cipher,
                            uint64_t cipher_len, void* out, uint8_t* frag_status, uint8_t* seg_status, int* ok) {
    if (!r || !ok) return bad_arg();
    *ok = 0;
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    RC_TRY(rs_narrow(r, "dm_restore_range_buffer"));
    if (!frags || !out) return fail(c, DM_ERR_INVALID, "dm_restore_range_buffer: null argument");
    CipherKey key;
    const bool ciph = cipher != nullptr || cipher_len != 0;
    Dev& d = c->devs[g];
    RangeCall q{r, &d, {}, segment, off, len, nullptr, ciph ? &key : nullptr, nullptr, nullptr};
    RC_TRY(range_check(r, nseg, size, segment, off, len, flags, ciph ? &key : nullptr, cipher, cipher_len, q.plan));
    RtStatus st(r, nseg);
    q.names = (flags & DM_RESTORE_VERIFY_FRAGMENTS) ? frag_names : nullptr;
    q.fst = st.fst.data();
    q.sst = st.sst.data();
    hipStream_t s = d.stream;
    const int total = r->k + r->m;
    const uint64_t frag = segment / (uint64_t)r->k, f00 = q.plan.seg0 * (uint64_t)total;
    uint64_t run0 = 0;
    auto given_of = [&](uint64_t t0, uint64_t ns, std::vector<uint8_t>& given) -> int {
        run0 = f00 + t0 * total;
        given.resize(ns * (uint64_t)total);
        for (uint64_t i = 0; i < given.size(); i++) given[i] = frags[run0 + i] != nullptr;
        return DM_OK;
    };
    const RangeLoad load = [&](const std::vector<RtLoad>& loads) -> int {
        for (const RtLoad& l : loads) HIP_TRY(hipMemcpyAsync(l.to, frags[run0 + l.idx], frag, hipMemcpyHostToDevice, s));
        return DM_OK;   // the launches follow on the same stream
    };
    int rc = begin_call(c, d, s);
    if (rc == DM_OK) rc = range_windows(q, q.plan.ntouched, given_of, load, out, ok);
    // no copy from or to the caller's memory stays queued, whichever way the call ends
    if (rc != DM_OK || !*ok) (void)hipStreamSynchronize(s);
    if (rc != DM_OK) *ok = 0;
    st.copy_out(frag_status, seg_status);
    return rc;
}

int dm_retrieve_range(dm_rs* r, const char* fragdir, const uint8_t* frag_names, uint64_t nseg, uint64_t size,
                      uint64_t segment, uint64_t off, uint64_t len, int flags, const void* cipher, uint64_t cipher_len,
                      void* out, uint8_t* frag_status, uint8_t* seg_status, int* ok) {
    if (!r || !ok) return bad_arg();
    *ok = 0;
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    RC_TRY(rs_narrow(r, "dm_retrieve_range"));
    if (!fragdir || !frag_names || !out) return fail(c, DM_ERR_INVALID, "dm_retrieve_range: null argument");
    CipherKey key;
    const bool ciph = cipher != nullptr || cipher_len != 0;
    Dev& d = c->devs[g];
    RangeCall q{r, &d, {}, segment, off, len, nullptr, ciph ? &key : nullptr, nullptr, nullptr};
    RC_TRY(range_check(r, nseg, size, segment, off, len, flags, ciph ? &key : nullptr, cipher, cipher_len, q.plan));
    RtStatus st(r, nseg);
    q.names = (flags & DM_RESTORE_VERIFY_FRAGMENTS) ? frag_names : nullptr;
    q.fst = st.fst.data();
    q.sst = st.sst.data();
    std::string dir = fragdir;
    while (dir.size() > 1 && dir.back() == '/') dir.pop_back();
    RsLane& L = rs_ln(r, d);
    const int total = r->k + r->m;
    const uint64_t frag = segment / (uint64_t)r->k, f00 = q.plan.seg0 * (uint64_t)total;
    // test hooks (env, read per call): small windows and slots exercise several windows and slot reuse
    const uint64_t win = std::max<uint64_t>(1, env_bytes("DEOSS_RT_WINDOW_BYTES", kRtWindowBytes) / segment);
    const uint64_t slot_cap = std::max(env_bytes("DEOSS_FP_SLOT_BYTES", kFpSlotBytes), frag);
    FpEvents ev;
    uint64_t next_slot = 0, run0 = 0;
    auto path = [&](uint64_t i) { return dir + "/" + hex32(frag_names + 32 * i); };
    auto given_of = [&](uint64_t t0, uint64_t ns, std::vector<uint8_t>& given) -> int {
        run0 = f00 + t0 * total;
        given.assign(ns * (uint64_t)total, 0);
        std::vector<uint8_t> wrong(given.size(), 0);
        for (uint64_t i = 0; i < given.size(); i++) {
            const std::string p = path(run0 + i);
            struct stat stt {};
            if (::stat(p.c_str(), &stt) != 0) {
                if (errno == ENOENT || errno == ENOTDIR) continue;   // not downloaded: absent
                return fail(c, DM_ERR_IO, "stat %s: %s", p.c_str(), go_errno(errno).c_str());
            }
            if (!S_ISREG(stt.st_mode) || (uint64_t)stt.st_size != frag) {
                wrong[i] = 1;   // not a fragment of this object's shape
                continue;
            }
            given[i] = 1;
        }
        // a file of the wrong length is bad where the range looks: a needed data fragment, or any
        // fragment of a segment that has to rebuild
        for (uint64_t t = 0; t < ns; t++) {
            const uint8_t* need = q.plan.need.data() + (t0 + t) * (uint64_t)r->k;
            bool rebuilds = false;
            for (int j = 0; j < r->k; j++) rebuilds |= need[j] && !given[t * total + j];
            for (int j = 0; j < total; j++)
                if (wrong[t * total + j] && (rebuilds || (j < r->k && need[j]))) st.fst[run0 + t * total + j] = kFragBad;
        }
        return DM_OK;
    };
    const RangeLoad load = [&](const std::vector<RtLoad>& loads) -> int {
        std::vector<std::string> paths;
        for (const RtLoad& l : loads) paths.push_back(path(run0 + l.idx));
        return rt_load(r, d, loads, paths, frag, slot_cap, ev, next_slot);
    };
    int rc = begin_call(c, d, d.stream);
    if (rc == DM_OK)
        for (auto& b : L.fp_slot)
            if (hipError_t e = b.ensure(slot_cap); e != hipSuccess) {
                rc = fail(c, e == hipErrorOutOfMemory ? DM_ERR_NOMEM : DM_ERR_HIP, "pinned slots: %s", hipGetErrorString(e));
                break;
            }
    if (rc == DM_OK)
        for (auto& e : ev.slot)
            if (hipError_t x = hipEventCreateWithFlags(&e, hipEventDisableTiming); x != hipSuccess) {
                rc = fail(c, DM_ERR_HIP, "hipEventCreateWithFlags: %s", hipGetErrorString(x));
                break;
            }
    if (rc == DM_OK) rc = range_windows(q, win, given_of, load, out, ok);
    if (rc != DM_OK) {   // a failed call may leave copies queued: none may land in a slot the next call fills
        (void)hipStreamSynchronize(d.copy);
        (void)hipStreamSynchronize(d.stream);
        *ok = 0;
    }
    if (d.data.cap > kFpKeepBytes) c->reaper.put(d.id, d.data);
    if (L.work.cap > kFpKeepBytes) c->reaper.put(d.id, L.work);
    st.copy_out(frag_status, seg_status);
    return rc;
}

}  // extern "C"
