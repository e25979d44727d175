// repair_capi.inl -- the storage side on the GPU: a segment's lost fragments, data or parity, from
// any `data` survivors (dm_rs_repair_*, dm_repair_buffer, dm_repair_files; include/deoss_merkle.h).
// Part of merkle_capi.hip (after restore_capi.inl; shares rs_desc_launch, rt_hash, rt_load, RtStatus
// and the pinned slots with the restore path).  Plans and a launch's descriptors are rs_plan.hpp
// (repair_plan, repair_add), the file writes are fp_files.hpp.
//
// Replaces, for a fragment that went missing, DeOSS's reFullProcessing (node/tracker.go:320-355,
// checkFileState): that one re-reads the object, needs the client's cipher and rewrites all 12
// fragments of every segment.  Fragments are ciphertext already and each is named by its own
// SHA-256, so here, per call (or per window of segments):
//   1. the first k usable fragments of every segment that needs anything go to HBM;
//   2. ONE repair launch writes the wanted fragments to scratch from those still-unverified inputs
//      (rs_restore_kernel when no segment has more than k outputs, else rs_repair_kernel);
//   3. ONE table-mode leaf launch hashes inputs and outputs together;
//   4. an output that equals its name is delivered; an input that does not is bad, its segment's
//      outputs are discarded and the next candidate takes its place in another round, of those
//      segments alone.

namespace {

constexpr uint64_t kRepairWindowBytes = 16ull << 30;  // dm_repair_files: loaded + rebuilt fragment bytes per GPU pass (a pass costs one 8 MiB chain, 122 ms, however few fragments it holds)
constexpr uint8_t kFragRebuilt = 4;                   // frag_status beyond the restore path's (rs_plan.hpp)

// Where a run of segments' fragments come from and where the rebuilt ones go (indices are
// t * total + j within the run).
struct RepairIo {
    virtual ~RepairIo() = default;
    virtual bool given(uint64_t i) const = 0;    // there is a fragment to load (it may still be bad)
    virtual bool wanted(uint64_t i) const = 0;   // deliver it when it is missing or bad
    virtual bool check(uint64_t i) const = 0;    // given, and verified even when no plan reads it
    virtual int load(const std::vector<RtLoad>& loads) = 0;          // to the device, complete on return
    virtual int deliver(uint64_t i, const uint8_t* dev) = 0;         // a rebuilt fragment that equals its name
    virtual int flush() = 0;                                         // every delivery so far has left the device
};

// Steps 1 - 4 for ns segments of one run: statuses to fst / sst (zero on entry).  A segment is worked
// on when a wanted fragment is not given or a given one is to be checked; another is not looked at.
// Rounds: a segment takes another round only when the last one condemned one of its fragments (a bad
// input, or a checked fragment that is bad and wanted), and with fewer than k left it ends as
// kSegTooFew, so a segment sees at most parity + 1 launches.
int repair_rounds(dm_rs* r, Dev& d, hipStream_t s, RepairIo& io, uint64_t ns, uint64_t frag, const uint8_t* names,
                  uint8_t* fst, uint8_t* sst) {
    dm_ctx* c = r->c;
    const int k = r->k, m = r->m, total = r->k + r->m;
    RsLane& L = rs_ln(r, d);
    enum : uint8_t { kNone, kGiven, kGood, kBad };
    std::vector<uint8_t> st(ns * (uint64_t)total, kNone), active(ns, 0), done(ns * (uint64_t)total, 0);
    std::vector<uint8_t*> slot(ns * (uint64_t)total, nullptr);   // where a loaded or rebuilt fragment lies
    std::vector<std::vector<uint8_t*>> freed(ns);
    uint64_t cap = 0, nactive = 0;
    for (uint64_t t = 0; t < ns; t++) {
        int ntarget = 0, ncheck = 0;
        for (int j = 0; j < total; j++) {
            const uint64_t i = t * total + j;
            if (io.given(i)) st[i] = kGiven;
            if (io.given(i) && io.check(i)) ncheck++;
            if (!io.given(i) && io.wanted(i)) ntarget++;
        }
        if (ntarget + ncheck == 0) continue;
        active[t] = 1;
        nactive++;
        cap += (uint64_t)std::min(total, k + ntarget + ncheck);   // inputs, targets, checked fragments beside the inputs
    }
    if (nactive == 0) return DM_OK;
    HIP_TRY(L.work.ensure(cap * frag + 16));
    // A bad fragment that is wanted keeps its slot for its rebuilt bytes, so the candidate that takes
    // its place as an input needs one more: those come from spill blocks, freed when the run ends.
    struct Spill {
        int dev;
        std::vector<void*> blocks;
        ~Spill() {
            for (void* p : blocks) dev_release(dev, p);   // waits for the device's queued work
        }
    } spill{d.id, {}};
    const uint64_t spill_slots = 16;
    uint64_t bump = 0, spill_left = 0;
    uint8_t* spill_at = nullptr;
    auto take = [&](uint64_t t) -> uint8_t* {
        if (!freed[t].empty()) {
            uint8_t* x = freed[t].back();
            freed[t].pop_back();
            return x;
        }
        if (bump < cap) return L.work.u8() + (bump++) * frag;
        if (spill_left == 0) {
            void* p = nullptr;
            if (dev_alloc(d.id, &p, spill_slots * frag) != hipSuccess) return nullptr;
            spill.blocks.push_back(p);
            spill_at = static_cast<uint8_t*>(p);
            spill_left = spill_slots;
        }
        spill_left--;
        uint8_t* x = spill_at;
        spill_at += frag;
        return x;
    };
    struct Seg {
        uint64_t t;
        int in[dm::kRsMaxIn];
        int out[dm::kRsMaxOut];
        int nout;
    };
    for (int round = 0; nactive > 0; round++) {
        RepairBatch b{r->mat.data(), k, m};
        std::vector<Seg> segs;
        std::vector<RtLoad> loads;
        for (uint64_t t = 0; t < ns; t++) {
            if (!active[t]) continue;
            Seg sg{};
            sg.t = t;
            int nin = 0;
            for (int j = 0; j < total && nin < k; j++)
                if (st[t * total + j] == kGiven || st[t * total + j] == kGood) sg.in[nin++] = j;
            if (nin < k) {
                sst[t] = kSegTooFew;
                active[t] = 0;
                nactive--;
                continue;
            }
            uint8_t* ptr[dm::kRsMaxIn + dm::kRsMaxOut] = {};
            uint8_t present[dm::kRsMaxIn + dm::kRsMaxOut] = {};
            bool room = true;
            for (int j = 0; j < total; j++) {
                const uint64_t i = t * total + j;
                const bool input = std::find(sg.in, sg.in + k, j) != sg.in + k;
                const bool target = io.wanted(i) && !done[i] && (st[i] == kNone || st[i] == kBad);
                const bool load = st[i] == kGiven && !slot[i] && (input || io.check(i));
                if ((load || target) && !slot[i] && !(slot[i] = take(t))) room = false;
                if (!room) break;
                if (load) loads.push_back({i, slot[i]});
                if (input || target) ptr[j] = slot[i];
                present[j] = input;
                if (target) sg.out[sg.nout++] = j;
            }
            if (!room) return fail(c, DM_ERR_NOMEM, "repair: out of device memory for fragments");
            RC_TRY(plan_status(c, repair_add(b, ptr, present), k));
            segs.push_back(sg);
        }
        if (segs.empty()) break;
        if (round > m) return fail(c, DM_ERR_INVALID, "repair: more than parity + 1 rounds");   // see above
        RC_TRY(io.load(loads));
        hipEvent_t* tr = timing_record(c, d);   // one record per round: one repair and one leaf launch
        if (tr) HIP_TRY(hipEventRecord(tr[0], s));
        RC_TRY(rs_desc_launch(r, d, s, b, frag / 16));
        std::vector<uint64_t> addrs;
        for (const RtLoad& l : loads) addrs.push_back(reinterpret_cast<uint64_t>(l.to));
        for (const Seg& sg : segs)
            for (int q = 0; q < sg.nout; q++)
                addrs.push_back(reinterpret_cast<uint64_t>(slot[sg.t * total + sg.out[q]]));
        std::vector<uint8_t> dig;
        RC_TRY(rt_hash(c, d, s, addrs, frag, dig));
        if (tr) {
            HIP_TRY(hipEventRecord(tr[1], s));
            HIP_TRY(hipEventRecord(tr[2], s));
        }
        for (size_t q = 0; q < loads.size(); q++) {
            const uint64_t i = loads[q].idx;
            const bool good = std::memcmp(dig.data() + 32 * q, names + 32 * i, 32) == 0;
            st[i] = good ? kGood : kBad;
            if (!good) {
                fst[i] = kFragBad;
                if (!io.wanted(i)) {   // wanted: its slot takes the rebuilt fragment
                    freed[i / total].push_back(slot[i]);
                    slot[i] = nullptr;
                }
            }
        }
        size_t q = loads.size();
        for (const Seg& sg : segs) {
            const uint64_t t = sg.t, f0 = t * total;
            const size_t q0 = q;
            q += (size_t)sg.nout;
            bool bad_in = false;
            for (int j = 0; j < k; j++) bad_in |= st[f0 + sg.in[j]] == kBad;
            if (bad_in) continue;   // its outputs are worth nothing; the next candidate, next round
            for (int e = 0; e < sg.nout; e++) {
                const uint64_t i = f0 + sg.out[e];
                if (std::memcmp(dig.data() + 32 * (q0 + e), names + 32 * i, 32) != 0) {
                    sst[t] = kSegMismatch;   // good inputs, another output: the names do not belong together
                    continue;
                }
                RC_TRY(io.deliver(i, slot[i]));
                done[i] = 1;
                fst[i] = kFragRebuilt;
            }
            bool more = false;   // a checked fragment found bad this round
            for (int j = 0; j < total; j++) {
                const uint64_t i = f0 + j;
                if (st[i] == kGood) fst[i] = std::find(sg.in, sg.in + k, j) != sg.in + k ? kFragUsed : kFragSpare;
                more |= st[i] == kBad && io.wanted(i) && !done[i] &&
                        std::find(sg.out, sg.out + sg.nout, j) == sg.out + sg.nout;
            }
            if (!more || sst[t] == kSegMismatch) {
                active[t] = 0;
                nactive--;
            }
        }
        RC_TRY(io.flush());   // before a slot is written again
    }
    for (uint64_t i = 0; i < ns * (uint64_t)total; i++)   // the good fragments of a segment with too few stay spare
        if (st[i] == kGood && fst[i] == kFragAbsent) fst[i] = kFragSpare;
    return DM_OK;
}

// *ok of a run: every fragment that was wanted and missing or bad has been delivered.
bool repair_complete(const RepairIo& io, uint64_t n, const uint8_t* fst) {
    for (uint64_t i = 0; i < n; i++)
        if (io.wanted(i) && fst[i] != kFragRebuilt && (!io.given(i) || fst[i] == kFragBad)) return false;
    return true;
}

struct RepairBufferIo : RepairIo {
    const void* const* frags;
    void* const* out;
    uint64_t frag;
    hipStream_t s;
    dm_ctx* c;
    bool given(uint64_t i) const override { return frags[i] != nullptr; }
    bool wanted(uint64_t i) const override { return out[i] != nullptr; }
    bool check(uint64_t i) const override { return frags[i] != nullptr && out[i] != nullptr; }
    int load(const std::vector<RtLoad>& loads) override {
        for (const RtLoad& l : loads) HIP_TRY(hipMemcpyAsync(l.to, frags[l.idx], frag, hipMemcpyHostToDevice, s));
        return DM_OK;   // the launches follow on the same stream
    }
    int deliver(uint64_t i, const uint8_t* dev) override {
        HIP_TRY(hipMemcpyAsync(out[i], dev, frag, hipMemcpyDeviceToHost, s));
        return DM_OK;
    }
    int flush() override {
        HIP_TRY(hipStreamSynchronize(s));
        return DM_OK;
    }
};

// The fragment files of a window of segments.  A name may have several owners (the zero tail of a
// padded last segment): one file serves them all, and a rebuilt one is written once.
struct RepairFilesIo : RepairIo {
    dm_rs* r;
    Dev* d;
    std::string dir, tmp_base;
    const uint8_t* names;          // of the window
    uint64_t frag, slot_cap;
    bool scrub;
    FpEvents* ev;
    uint64_t* next_slot;
    std::vector<uint8_t> have;                       // the window's fragments whose file exists with the right length
    std::map<std::string, int>* written;             // names this call has rebuilt -> 1
    std::vector<std::pair<uint64_t, const uint8_t*>> queue;
    std::vector<std::string>* temps;                 // temporaries that exist right now
    uint64_t nrebuilt = 0;

    std::string path(uint64_t i) const { return dir + "/" + hex32(names + 32 * i); }
    bool given(uint64_t i) const override { return have[i] != 0; }
    bool wanted(uint64_t) const override { return true; }   // whatever is found missing or bad is rebuilt
    bool check(uint64_t i) const override { return have[i] && scrub; }
    int load(const std::vector<RtLoad>& loads) override {
        std::vector<std::string> paths;
        for (const RtLoad& l : loads) paths.push_back(path(l.idx));
        return rt_load(r, *d, loads, paths, frag, slot_cap, *ev, *next_slot);
    }
    int deliver(uint64_t i, const uint8_t* dev) override {
        queue.emplace_back(i, dev);
        return DM_OK;
    }
    // Device -> pinned slot -> temporary file -> its hex name, a slot's worth at a time.
    int flush() override {
        dm_ctx* c = r->c;
        RsLane& L = rs_ln(r, *d);
        hipStream_t s = d->stream;
        const uint64_t per = std::max<uint64_t>(1, slot_cap / frag);
        std::vector<std::pair<uint64_t, const uint8_t*>> todo;
        for (const auto& e : queue) {   // one owner per name writes
            const std::string nm(reinterpret_cast<const char*>(names + 32 * e.first), 32);
            if (written->emplace(nm, 1).second) todo.push_back(e);
        }
        queue.clear();
        for (size_t g0 = 0; g0 < todo.size(); g0 += per) {
            const size_t n = std::min<size_t>(per, todo.size() - g0);
            const int sl = (int)((*next_slot)++ % kFpSlots);
            HIP_TRY(hipEventSynchronize(ev->slot[sl]));
            uint8_t* buf = L.fp_slot[sl].u8();
            for (size_t q = 0; q < n; q++)
                HIP_TRY(hipMemcpyAsync(buf + q * frag, todo[g0 + q].second, frag, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            std::vector<FpFile> files;
            for (size_t q = 0; q < n; q++) {
                temps->push_back(tmp_base + std::to_string((unsigned long long)temps->size()));
                files.push_back({buf + q * frag, frag, temps->back()});
            }
            SlotWrites w;
            w.start(files);
            const std::string err = w.wait();
            if (!err.empty()) return fail(c, DM_ERR_IO, "%s", err.c_str());
            for (size_t q = 0; q < n; q++) {   // the digest matched before the bytes left the device
                std::string& tmp = (*temps)[temps->size() - n + q];
                const std::string to = path(todo[g0 + q].first);
                if (::rename(tmp.c_str(), to.c_str()) != 0)
                    return fail(c, DM_ERR_IO, "rename %s %s: %s", tmp.c_str(), to.c_str(), go_errno(errno).c_str());
                tmp.clear();
                nrebuilt++;
            }
        }
        return DM_OK;
    }
};

// Everything of dm_repair_files but the temporaries' fate.
int repair_windows(dm_rs* r, Dev& d, const std::string& dir, const uint8_t* frag_names, uint64_t nseg, uint64_t segment,
                   int flags, uint8_t* fst, uint8_t* sst, std::vector<std::string>& temps, uint64_t* nrebuilt, int* ok) {
    dm_ctx* c = r->c;
    RsLane& L = rs_ln(r, d);
    hipStream_t s = d.stream;
    RC_TRY(begin_call(c, d, s));
    const int k = r->k, total = r->k + r->m;
    const uint64_t frag = segment / (uint64_t)k;
    // test hooks (env, read per call): small windows and slots exercise several windows and slot reuse
    const uint64_t budget = std::max<uint64_t>(1, env_bytes("DEOSS_REPAIR_WINDOW_BYTES", kRepairWindowBytes) / frag);
    const uint64_t slot_cap = std::max(env_bytes("DEOSS_FP_SLOT_BYTES", kFpSlotBytes), frag);
    const bool scrub = (flags & DM_REPAIR_SCRUB) != 0;
    FpEvents ev;
    uint64_t next_slot = 0;
    bool slots_ready = false;
    std::map<std::string, int> written;
    const std::string tmp_base = dir + "/.dm-rp-" + std::to_string((long long)::getpid()) + "-" +
                                 std::to_string((unsigned long long)g_fp_seq++) + "-";
    bool all = true;
    uint64_t rebuilt = 0;
    for (uint64_t w0 = 0; w0 < nseg;) {
        // the window: segments while the fragments they load and rebuild fit the budget (one at least)
        RepairFilesIo io;
        uint64_t ns = 0, cost = 0;
        std::vector<std::pair<uint64_t, uint8_t>> rebuilt_earlier;
        while (w0 + ns < nseg) {
            std::vector<uint8_t> have((size_t)total, 0);
            std::vector<std::pair<uint64_t, uint8_t>> early;
            int missing = 0;
            for (int j = 0; j < total; j++) {
                const uint8_t* nm = frag_names + 32 * ((w0 + ns) * total + j);
                const std::string p = dir + "/" + hex32(nm);
                struct stat stt {};
                if (::stat(p.c_str(), &stt) != 0) {
                    if (errno != ENOENT && errno != ENOTDIR)
                        return fail(c, DM_ERR_IO, "stat %s: %s", p.c_str(), go_errno(errno).c_str());
                } else if (S_ISREG(stt.st_mode) && (uint64_t)stt.st_size == frag) {
                    have[j] = 1;
                    if (written.count(std::string(reinterpret_cast<const char*>(nm), 32))) early.emplace_back(ns * total + j, 1);
                }
                missing += !have[j];
            }
            const uint64_t mine = scrub ? (uint64_t)total : missing ? (uint64_t)(k + missing) : 0;
            if (ns > 0 && cost + mine > budget) break;
            cost += mine;
            rebuilt_earlier.insert(rebuilt_earlier.end(), early.begin(), early.end());
            io.have.insert(io.have.end(), have.begin(), have.end());
            ns++;
        }
        uint8_t* wf = fst + w0 * total;
        if (cost) {
            if (!slots_ready) {
                for (auto& b : L.fp_slot) HIP_TRY(b.ensure(slot_cap));
                for (auto& e : ev.slot) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                slots_ready = true;
            }
            io.r = r;
            io.d = &d;
            io.dir = dir;
            io.tmp_base = tmp_base;
            io.names = frag_names + 32 * w0 * total;
            io.frag = frag;
            io.slot_cap = slot_cap;
            io.scrub = scrub;
            io.ev = &ev;
            io.next_slot = &next_slot;
            io.written = &written;
            io.temps = &temps;
            RC_TRY(repair_rounds(r, d, s, io, ns, frag, io.names, wf, sst + w0));
            rebuilt += io.nrebuilt;
            // an owner that could not rebuild a name another owner did: the file is there
            for (uint64_t i = 0; i < ns * (uint64_t)total; i++)
                if (io.wanted(i) && (!io.given(i) || wf[i] == kFragBad) &&
                    written.count(std::string(reinterpret_cast<const char*>(io.names + 32 * i), 32)))
                    wf[i] = kFragRebuilt;
            if (!repair_complete(io, ns * (uint64_t)total, wf)) all = false;
        }
        // an owner in a later window of a name an earlier window rebuilt
        for (const auto& e : rebuilt_earlier)
            if (wf[e.first] == kFragAbsent) wf[e.first] = kFragRebuilt;
        w0 += ns;
    }
    if (nrebuilt) *nrebuilt = rebuilt;
    *ok = all ? 1 : 0;
    return DM_OK;
}

// The arguments the verified repair calls share.
int repair_check(dm_rs* r, uint64_t nseg, uint64_t segment) {
    if (nseg == 0) return fail(r->c, DM_ERR_EMPTY, "Empty data");
    return process_check(r, 1, segment);
}

}  // namespace

extern "C" {

int dm_rs_repair_plan(int data, int parity, const uint8_t* present, const uint8_t* want, int* inputs, int* outputs,
                      uint8_t* rows, int* nout) {
    if (!present || !inputs || !outputs || !rows || !nout) return bad_arg();
    if (data < 1 || data > dm::kRsMaxIn || parity < 1 || parity > dm::kRsMaxOut)
        return fail(nullptr, DM_ERR_INVALID, "shard counts: 1 <= data <= %d, 1 <= parity <= %d", dm::kRsMaxIn,
                    dm::kRsMaxOut);
    std::vector<uint8_t> mat;
    {
        std::lock_guard<std::mutex> lk(g_plan_mu);
        std::vector<uint8_t>& cached = g_plan_mats[data * 16 + parity];
        if (cached.empty() && !rs_build_matrix(data, parity, cached))
            return fail(nullptr, DM_ERR_INVALID, "singular Vandermonde top");
        mat = cached;
    }
    RsPlan p;
    RC_TRY(plan_status(nullptr, repair_plan(mat.data(), data, parity, present, want, p), data));
    std::memcpy(inputs, p.inputs, sizeof(int) * (size_t)data);
    std::memcpy(outputs, p.outputs, sizeof(int) * (size_t)p.nout);
    std::memcpy(rows, p.rows, (size_t)p.nout * (size_t)data);
    *nout = p.nout;
    return DM_OK;
}

int dm_rs_repair_device_async(dm_rs* r, void* const* dev_frags, const uint8_t* present, uint64_t nseg, uint64_t frag,
                              void* stream) {
    if (!r) return bad_arg();
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    RC_TRY(rs_narrow(r, "dm_rs_repair_device_async"));
    const int k = r->k, total = r->k + r->m;
    if (!dev_frags || !present || nseg == 0 || frag == 0 || frag % 16)
        return fail(c, DM_ERR_INVALID,
                    "dm_rs_repair_device_async: need fragments, their presence and a fragment size that is a "
                    "non-zero multiple of 16");
    for (uint64_t i = 0; i < nseg * (uint64_t)total; i++)
        if (!is_aligned16(dev_frags[i]))
            return fail(c, DM_ERR_INVALID, "dm_rs_repair_device_async: fragment %llu of segment %llu not 16-byte aligned",
                        (unsigned long long)(i % total), (unsigned long long)(i / total));
    RepairBatch b{r->mat.data(), k, r->m};   // every plan first: a segment with too few fragments fails the call before any launch
    b.desc.reserve(nseg);
    for (uint64_t t = 0; t < nseg; t++)
        RC_TRY(plan_status(c, repair_add(b, reinterpret_cast<uint8_t* const*>(dev_frags) + t * total, present + t * total), k));
    Dev& d = c->devs[g];
    hipStream_t s = pick_stream(d, stream);
    RC_TRY(begin_call(c, d, s));
    return rs_desc_launch(r, d, s, b, frag / 16);
}

int dm_repair_buffer(dm_rs* r, const void* const* frags, void* const* out, const uint8_t* frag_names, uint64_t nseg,
                     uint64_t segment, uint8_t* frag_status, uint8_t* seg_status, int* ok) {
    if (!r || !ok) return bad_arg();
    *ok = 0;
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    RC_TRY(rs_narrow(r, "dm_repair_buffer"));
    if (!frags || !out || !frag_names) return fail(c, DM_ERR_INVALID, "dm_repair_buffer: null argument");
    RC_TRY(repair_check(r, nseg, segment));
    Dev& d = c->devs[g];
    hipStream_t s = d.stream;
    RtStatus st(r, nseg);
    RepairBufferIo io;
    io.frags = frags;
    io.out = out;
    io.frag = segment / (uint64_t)r->k;
    io.s = s;
    io.c = c;
    int rc = begin_call(c, d, s);
    if (rc == DM_OK) rc = repair_rounds(r, d, s, io, nseg, io.frag, frag_names, st.fst.data(), st.sst.data());
    // no copy from or to the caller's memory stays queued, whichever way the call ends
    if (rc != DM_OK) (void)hipStreamSynchronize(s);
    else *ok = repair_complete(io, nseg * (uint64_t)(r->k + r->m), st.fst.data()) ? 1 : 0;
    st.copy_out(frag_status, seg_status);
    return rc;
}

int dm_repair_files(dm_rs* r, const char* fragdir, const uint8_t* frag_names, uint64_t nseg, uint64_t segment, int flags,
                    uint8_t* frag_status, uint8_t* seg_status, uint64_t* nrebuilt, int* ok) {
    if (!r || !ok) return bad_arg();
    *ok = 0;
    if (nrebuilt) *nrebuilt = 0;
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    RC_TRY(rs_narrow(r, "dm_repair_files"));
    if (!fragdir || !frag_names) return fail(c, DM_ERR_INVALID, "dm_repair_files: null argument");
    RC_TRY(repair_check(r, nseg, segment));
    std::string dir = fragdir;
    while (dir.size() > 1 && dir.back() == '/') dir.pop_back();
    Dev& d = c->devs[g];
    RtStatus st(r, nseg);
    std::vector<std::string> temps;
    const int rc = repair_windows(r, d, dir, frag_names, nseg, segment, flags, st.fst.data(), st.sst.data(), temps,
                                  nrebuilt, ok);
    if (rc != DM_OK) {   // a failed call may leave copies queued: none may land in a slot the next call fills
        (void)hipStreamSynchronize(d.copy);
        (void)hipStreamSynchronize(d.stream);
        *ok = 0;
    }
    for (const std::string& t : temps)   // no temporary survives, whichever way the call ends
        if (!t.empty()) ::unlink(t.c_str());
    if (rs_ln(r, d).work.cap > kFpKeepBytes) c->reaper.put(d.id, rs_ln(r, d).work);
    st.copy_out(frag_status, seg_status);
    return rc;
}

}  // extern "C"
