// broadphase.hip — DeviceBroadphase, the host side of the sweep-and-prune broadphase: what an update reserves, queues and reads back
// (the kernels, the sweep's views and the layout notes: broadphase_kernels.h; the C exports: c_api_broadphase.hip).
#include "handles.h"
#include "device_radix.h"
#include "broadphase_kernels.h"

namespace phx {

DeviceBroadphase::~DeviceBroadphase()
{
    if (hipSetDevice(device_) != hipSuccess) return;
    if (stream_) (void)hipStreamSynchronize(stream_);
    // (device buffers are DevBuf members: freed with the object)
    if (stream_) (void)hipStreamDestroy(stream_);
}

int DeviceBroadphase::init()
{
    PHX_TRY(use_device(device_));
    PHX_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    PHX_TRY(small_.reserve(SMALL_WORDS));
    PHX_TRY(erase_count_.reserve(1));
    PHX_HIP(hipMemsetAsync(erase_count_.p, 0, sizeof(int), stream_));
    return clear();
}

int DeviceBroadphase::exclusive_scan(unsigned* data, int count, unsigned* total_out)
{
    return device_exclusive_scan(data, count, total_out, scan_tiles_, stream_);
}

int DeviceBroadphase::resize_table(unsigned want_cap)
{
    unsigned cap = 1024;
    while (cap < want_cap) cap <<= 1;
    DevBuf<unsigned long long> fresh;
    PHX_TRY(fresh.reserve(cap));
    PHX_HIP(hipMemsetAsync(fresh.p, 0xFF, (size_t)cap * sizeof(unsigned long long), stream_));
    if (table_.p && table_cap_) {
        hipLaunchKernelGGL(k_ps_rehash, dim3(grid_for((int)table_cap_)), dim3(256), 0, stream_, table_.p, table_cap_, fresh.p, cap - 1);
        PHX_HIP(hipGetLastError());
    }
    PHX_HIP(hipStreamSynchronize(stream_));
    table_ = std::move(fresh);
    table_cap_ = cap;
    tombstones_ = 0;
    return PHX_OK;
}

int DeviceBroadphase::clear()
{
    PHX_TRY(use_device(device_));
    table_.release();
    table_cap_ = 0;
    set_size_ = 0;
    tombstones_ = 0;
    if (erase_unchecked_) { erase_unchecked_ = 0; PHX_HIP(hipMemsetAsync(erase_count_.p, 0, sizeof(int), stream_)); }
    return resize_table(1024);
}

int DeviceBroadphase::update_device(const phx_rigid_body* d_bodies, int n)
{
    PHX_TRY(use_device(device_));
    PHX_REQUIRE(n >= 0 && (n == 0 || d_bodies), "bad body array");
    PHX_TRY(st_aabb_.reserve(std::max(n, 1)));
    if (n) hipLaunchKernelGGL(k_extract_aabb, dim3(grid_for(n)), dim3(256), 0, stream_, d_bodies, n, st_aabb_.p);
    PHX_HIP(hipGetLastError());
    return update_resident(st_aabb_.p, n);
}

// what the stages of one update hand on
struct DeviceBroadphase::Update {
    int n;
    const uint4* filters;                   // (null: unfiltered)
    const ExclusionView* exclusions;        // (null: none)
    int chunk_cap = 0, chunk_grid = 1;      // the hub chunk list's slots (grows on demand: count_new_pairs), the workgroups of the count pass over them
    SweepView v{};
    unsigned long long small[SMALL_WORDS] = {0};      // small_ as the count pass's readback found it

    int chunks_needed() const { return (int)(small[SMALL_CHUNKS_NEEDED] & 0xFFFFFFFFull); }
    unsigned new_pairs() const { return (unsigned)small[SMALL_NEW_PAIRS]; }
    bool cache_overflowed() const { return (small[SMALL_CACHE_OVERFLOW] & 0xFFFFFFFFull) != 0; }
    // the sweep's four instantiations: plain, filtered, excluded, both — `f` gets `v` as the view the world's settings pick
    template <class F> void with_view(F f) const
    {
        if (filters && exclusions) f(FilteredExcludedSweepView{{v, filters}, *exclusions});
        else if (filters) f(FilteredSweepView{v, filters});
        else if (exclusions) f(ExcludedSweepView{v, *exclusions});
        else f(v);
    }
};

int DeviceBroadphase::update_resident(const float4* d_bodies, int n, const StepPrologue* prologue, const std::function<int()>* while_waiting, const MailCarrier* carrier,
                                      const uint4* filters, const ExclusionView* exclusions)
{
    PHX_TRY(use_device(device_));
    PHX_REQUIRE(n >= 0 && (n == 0 || d_bodies), "bad body array");
    n_ = n;
    last_new_ = 0;
    stats_ = phx_broadphase_stats{};
    Update u{n, filters, exclusions};
    PHX_TRY(reserve_update(u));
    if (n == 0) return empty_update(prologue);
    PHX_TRY(sort(d_bodies, prologue, u));
    PHX_TRY(count_new_pairs(u, while_waiting, carrier));      // sweep: count -> scan ...
    PHX_TRY(emit_new_pairs(u));                               // ... -> emit
    // (not synchronised here: what follows on this stream — insertions' consumers, the next phase of a World — is ordered
    //  behind it; get_stats / get_new_pairs / get_sorted synchronise before they read)
    stats_.set_size = (int)set_size_;
    have_update_ = true;
    ms_pending_ = true;
    return PHX_OK;
}

int DeviceBroadphase::reserve_update(Update& u)
{
    const int n = u.n;
    for (int k = 0; k < 2; ++k) { PHX_TRY(keys_[k].reserve(std::max(n, 1))); PHX_TRY(idx_[k].reserve(std::max(n, 1))); }
    PHX_TRY(hist_.reserve(radix_hist_words(n)));
    u.chunk_cap = std::max<int>((int)chunks_.cap, div_up(std::max(n, 1), HUB_CHUNK) * 8 + 64);
    PHX_TRY(chunks_.reserve(u.chunk_cap));
    PHX_TRY(chunk_count_.reserve(u.chunk_cap));
    PHX_TRY(entries_.reserve(std::max(n, 1)));
    PHX_TRY(row_count_.reserve(std::max(n, 1) + 1));
    PHX_TRY(row_cache_.reserve((size_t)std::max(n, 1) * ROW_CACHE));
    // keep the table at most half full counting tombstones, before anything reads it
    if ((unsigned long long)(set_size_ + tombstones_) * 2 > table_cap_) PHX_TRY(resize_table((unsigned)std::max<long long>(4 * set_size_, 1024)));
    return stamps_.reserve(2);
}

// no bodies: nothing to sort or sweep, only what the update's first kernel would have cleared
int DeviceBroadphase::empty_update(const StepPrologue* prologue)
{
    if (prologue) PHX_HIP(hipMemsetAsync(prologue->counters, 0, 8 * sizeof(unsigned), stream_));
    PHX_HIP(hipMemsetAsync(stamps_.p, 0, 2 * sizeof(unsigned long long), stream_));
    PHX_HIP(hipStreamSynchronize(stream_));
    stats_.set_size = (int)set_size_; have_update_ = true; ms_pending_ = true;
    return PHX_OK;
}

// The sort.  With last update's splitters on record (same body count): the two-level sort of splitter_sort.h — three launches;
// otherwise (first update, another body count, buckets that got out of balance) the stable LSD radix sort — eleven — whose
// gather leaves the splitters for the next update.  Both produce the reference's sorted sequence (ref: base/RadixSort.h:28-95).
// Bodies appended since the splitters were taken (bodies_appended; at most as many again) are dealt into the buckets of the splitters
// on record (`deal`); the next splitters are taken at the new count's stride all the same.
// Either sort's first kernel takes the update's head along; the sorted records are left in keys_ / idx_[sorted_] and entries_.
int DeviceBroadphase::sort(const float4* d_bodies, const StepPrologue* prologue, const Update& u)
{
    const int n = u.n;
    UpdateHead head{};
    if (prologue) { head.vel = prologue->vel; head.mpos = prologue->mpos; head.accel = prologue->accel; head.counters = prologue->counters; head.gravity = prologue->gravity; head.dt = prologue->dt; }
    head.small = small_.p; head.nsmall = SMALL_WORDS; head.chunk_count = chunk_count_.p; head.nchunks = u.chunk_cap; head.stamps = stamps_.p;
    const int buckets = ss_buckets(n);
    const bool appended = splitters_n_ == n && splitters_from_ > 0 && splitters_from_ < n;
    const int deal = appended ? ss_buckets(splitters_from_) : buckets;
    PHX_TRY(splitters_.reserve(SS_MAX_BUCKETS)); PHX_TRY(ss_stats_.reserve(2));
    static const bool no_split = getenv("PHX_NO_SPLIT_SORT") != nullptr;      // A/B measurements, tests
    const bool split = !no_split && buckets <= SS_MAX_BUCKETS && (buckets == 1 || (splitters_n_ == n && !split_unbalanced_ && (!appended || n <= 2 * splitters_from_)));
    int src = 0;
    if (split) {
        if (!ss_count_.p) { PHX_TRY(ss_count_.reserve(2 * SS_MAX_BUCKETS)); PHX_HIP(hipMemsetAsync(ss_count_.p, 0, ss_count_.cap * sizeof(unsigned), stream_)); }
        PHX_TRY(ss_base_.reserve(SS_MAX_BUCKETS + 1)); PHX_TRY(bucket_of_.reserve(n)); PHX_TRY(bucketed_.reserve(n));
        SplitSortView sv{};
        sv.aabb = d_bodies; sv.n = n; sv.buckets = deal; sv.stride = ss_stride(n); sv.splitters = splitters_.p; sv.keys = keys_[0].p; sv.bucket_of = bucket_of_.p;
        sv.count = ss_count_.p; sv.cursor = ss_count_.p + SS_MAX_BUCKETS; sv.base = ss_base_.p; sv.bucketed = bucketed_.p;
        sv.keys_out = keys_[1].p; sv.idx_out = idx_[1].p; sv.entries = entries_.p; sv.next_splitters = splitters_.p; sv.max_bucket = ss_stats_.p;
        const bool large = ss_tile_items(deal) == SS_ITEMS_LARGE;
        const dim3 tiles(div_up(n, SS_TILE_T * ss_tile_items(deal)));
        const auto keys_buckets = prologue ? (large ? k_keys_buckets<true, SS_ITEMS_LARGE> : k_keys_buckets<true, SS_ITEMS_SMALL>)
                                           : (large ? k_keys_buckets<false, SS_ITEMS_LARGE> : k_keys_buckets<false, SS_ITEMS_SMALL>);
        hipLaunchKernelGGL(keys_buckets, tiles, dim3(SS_TILE_T), 0, stream_, sv, head);
        if (large) hipLaunchKernelGGL((k_bucket_scatter<SS_ITEMS_LARGE>), tiles, dim3(SS_TILE_T), 0, stream_, sv);
        else hipLaunchKernelGGL((k_bucket_scatter<SS_ITEMS_SMALL>), tiles, dim3(SS_TILE_T), 0, stream_, sv);
        // (the small LDS shape while the last update's largest bucket left room: all buckets resident at once)
        if (ss_last_max_ <= (unsigned)SS_LDS_SMALL_LIMIT) hipLaunchKernelGGL((k_bucket_sort<SS_LDS_SMALL>), dim3(deal), dim3(SS_SORT_T), 0, stream_, sv);
        else hipLaunchKernelGGL((k_bucket_sort<SS_LDS_RECORDS>), dim3(deal), dim3(SS_SORT_T), 0, stream_, sv);
        src = 1;
    } else {
        const auto build_keys = prologue ? k_build_keys<true> : k_build_keys<false>;
        hipLaunchKernelGGL(build_keys, dim3(grid_for(n)), dim3(256), 0, stream_, d_bodies, n, keys_[0].p, idx_[0].p, head);
        PHX_TRY(device_radix_sort_pairs(keys_[0].p, idx_[0].p, keys_[1].p, idx_[1].p, n, 32, hist_.p, scan_tiles_, stream_, &src));
        hipLaunchKernelGGL(k_gather_entries, dim3(grid_for(n)), dim3(256), 0, stream_, d_bodies, (const unsigned*)keys_[src].p, (const unsigned*)idx_[src].p, n, entries_.p, splitters_.p, ss_stride(n));
        PHX_HIP(hipMemsetAsync(ss_stats_.p, 0, sizeof(unsigned), stream_));
        split_unbalanced_ = false;
    }
    sorted_ = src;
    splitters_n_ = n; splitters_from_ = n;
    split_sorted_ = split;
    return PHX_OK;
}

// The count pass: new pairs per row and per hub chunk, the chunks' bases, the scan of the rows' counts — and the update's one readback,
// small_ into u.small.  Counted a second time, once, if the hub chunk list proved too short.
int DeviceBroadphase::count_new_pairs(Update& u, const std::function<int()>* while_waiting, const MailCarrier* carrier)
{
    const int n = u.n;
    const bool split = split_sorted_;
    SweepView& v = u.v;
    v.entries = entries_.p; v.idx = idx_[sorted_].p; v.n = n; v.table = table_.p; v.mask = table_cap_ - 1;
    v.row_count = row_count_.p; v.row_cache = row_cache_.p; v.cache_overflow = reinterpret_cast<int*>(small_.p + SMALL_CACHE_OVERFLOW);
    v.n_chunks = reinterpret_cast<int*>(small_.p + SMALL_CHUNKS_NEEDED);
    v.counters = small_.p + SMALL_STATS;
    for (int attempt = 0;; ++attempt) {
        v.chunks = chunks_.p; v.chunk_count = chunk_count_.p; v.chunk_cap = u.chunk_cap;
        u.chunk_grid = std::min(u.chunk_cap, 2048);
        u.with_view([&](const auto& sv) {
            using V = std::decay_t<decltype(sv)>;
            hipLaunchKernelGGL((k_sweep_rows<false, V>), dim3(grid_for(n)), dim3(256), 0, stream_, sv, (const unsigned*)nullptr, (uint2*)nullptr, 0u);
            hipLaunchKernelGGL((k_sweep_chunks_count<V>), dim3(u.chunk_grid), dim3(256), 0, stream_, sv);
        });
        // chunk counts -> per-row bases and the hub rows' totals (one small workgroup)
        PHX_TRY(chunk_scan_.reserve(u.chunk_cap + 1));
        hipLaunchKernelGGL(k_chunk_bases, dim3(1), dim3(1024), 0, stream_, v, chunk_scan_.p);
        PHX_TRY(exclusive_scan(row_count_.p, n, reinterpret_cast<unsigned*>(small_.p + SMALL_NEW_PAIRS)));
        PHX_HIP(hipGetLastError());
        int erased = 0;
        PHX_TRY(queue_erase_check(&erased));
        PHX_TRY(rb_.add(u.small, small_.p, sizeof u.small, stream_));
        unsigned max_bucket = 0;
        if (split) PHX_TRY(rb_.add(&max_bucket, ss_stats_.p, sizeof max_bucket, stream_));
        PHX_TRY(rb_.wait(stream_, stamps_.p + 1, attempt == 0 ? while_waiting : nullptr, attempt == 0 ? carrier : nullptr));
        PHX_TRY(settle_erase_check(erased));
        ss_last_max_ = split ? max_bucket : 0u;
        if (split && max_bucket > (unsigned)(4 * ss_stride(n))) split_unbalanced_ = true;      // (stale splitters: the next update sorts the long way and takes fresh ones)
        const int needed = u.chunks_needed();
        if (needed <= u.chunk_cap) break;
        // pathological overlap (many rows each spanning thousands of candidates): the chunk list was too short.
        // Its exact length is now known; grow it and redo the count pass.
        if (attempt) { set_error("broadphase: hub chunk list overflow twice (%d chunks)", needed); return PHX_ERR_CAPACITY; }
        u.chunk_cap = needed + 64;
        PHX_TRY(chunks_.reserve(u.chunk_cap));
        PHX_TRY(chunk_count_.reserve(u.chunk_cap));
        PHX_HIP(hipMemsetAsync(small_.p, 0, SMALL_WORDS * sizeof(unsigned long long), stream_));
        PHX_HIP(hipMemsetAsync(chunk_count_.p, 0, (size_t)u.chunk_cap * sizeof(unsigned), stream_));
    }
    stats_.candidate_tests = 0; stats_.overlapping_pairs = 0;
    for (int k = 0; k < STAT_SLOTS; ++k) { stats_.candidate_tests += (long long)u.small[SMALL_STATS + 2 * k]; stats_.overlapping_pairs += (long long)u.small[SMALL_STATS + 2 * k + 1]; }
    stats_.new_pairs = (int)u.new_pairs();
    last_new_ = (int)u.new_pairs();
    return PHX_OK;
}

// The emit pass: the counted pairs into new_pairs_ in the reference's order, and into the pair set (grown first if they would fill it).
int DeviceBroadphase::emit_new_pairs(Update& u)
{
    const int n = u.n;
    const unsigned total = u.new_pairs();
    if (!total) return PHX_OK;
    PHX_TRY(new_pairs_.reserve(total));
    if ((unsigned long long)(set_size_ + tombstones_ + (long long)total) * 2 > table_cap_)
        PHX_TRY(resize_table((unsigned)std::min<long long>(4ll * (set_size_ + (long long)total), 1ll << 30)));
    u.v.table = table_.p; u.v.mask = table_cap_ - 1;
    const int row_blocks = grid_for(n), chunk_blocks = u.chunks_needed() ? std::min(u.chunks_needed(), u.chunk_grid) : 0;
    u.with_view([&](const auto& sv) {
        using V = std::decay_t<decltype(sv)>;
        hipLaunchKernelGGL((k_emit_pairs<V>), dim3(row_blocks + chunk_blocks), dim3(256), 0, stream_, sv, (const unsigned*)row_count_.p, new_pairs_.p, total, row_blocks);
        // some row found more than ROW_CACHE new pairs: those rows are rescanned (with the count pass's filter and exclusions)
        if (u.cache_overflowed()) hipLaunchKernelGGL((k_sweep_rows<true, V>), dim3(grid_for(n)), dim3(256), 0, stream_, sv, (const unsigned*)row_count_.p, new_pairs_.p, total);
    });
    // ref: Collider.cpp:313 / :341 — the emitted pairs join the persistent set
    hipLaunchKernelGGL(k_ps_insert, dim3(grid_for((int)total)), dim3(256), 0, stream_, table_.p, table_cap_ - 1, (const uint2*)new_pairs_.p, (int)total, stamps_.p + 1);
    PHX_HIP(hipGetLastError());
    set_size_ += total;
    return PHX_OK;
}

int DeviceBroadphase::update_host(const phx_rigid_body* bodies, int n, uint32_t* new_pairs, int cap, int* count)
{
    PHX_TRY(use_device(device_));
    PHX_REQUIRE(n >= 0 && (n == 0 || bodies), "bad body array");
    PHX_TRY(st_bodies_.reserve(std::max(n, 1)));
    if (n) PHX_HIP(hipMemcpyAsync(st_bodies_.p, bodies, (size_t)n * sizeof(phx_rigid_body), hipMemcpyHostToDevice, stream_));
    PHX_TRY(update_device(st_bodies_.p, n));
    PHX_HIP(hipStreamSynchronize(stream_));
    return get_new_pairs(new_pairs, cap, count);
}

// the getters' refusal before the first update
int DeviceBroadphase::require_update() const
{
    if (!have_update_) { set_error("no broadphase update has run yet"); return PHX_ERR_STATE; }
    return PHX_OK;
}

int DeviceBroadphase::get_new_pairs(uint32_t* out, int cap, int* count)
{
    PHX_TRY(require_update());
    if (count) *count = last_new_;
    if (!out) return PHX_OK;
    if (cap < last_new_) { set_error("new-pair buffer too small: need %d", last_new_); return PHX_ERR_CAPACITY; }
    PHX_TRY(use_device(device_));
    PHX_HIP(hipStreamSynchronize(stream_));
    if (last_new_) PHX_HIP(hipMemcpy(out, new_pairs_.p, (size_t)last_new_ * sizeof(uint2), hipMemcpyDeviceToHost));
    return PHX_OK;
}

int DeviceBroadphase::get_sorted(phx_sort_entry* sorted, phx_broadphase_entry* entries, int cap)
{
    PHX_TRY(require_update());
    if (cap < n_) { set_error("sorted buffers too small: need %d", n_); return PHX_ERR_CAPACITY; }
    PHX_TRY(use_device(device_));
    if (!n_) return PHX_OK;
    DevBuf<phx_broadphase_entry> de;
    DevBuf<phx_sort_entry> ds;
    PHX_TRY(de.reserve(n_));
    PHX_TRY(ds.reserve(n_));
    hipLaunchKernelGGL(k_entries_to_aos, dim3(grid_for(n_)), dim3(256), 0, stream_, (const float4*)entries_.p, (const unsigned*)keys_[sorted_].p,
                       (const unsigned*)idx_[sorted_].p, n_, de.p, ds.p);
    PHX_HIP(hipGetLastError());
    if (entries) PHX_HIP(hipMemcpyAsync(entries, de.p, (size_t)n_ * sizeof(phx_broadphase_entry), hipMemcpyDeviceToHost, stream_));
    if (sorted) PHX_HIP(hipMemcpyAsync(sorted, ds.p, (size_t)n_ * sizeof(phx_sort_entry), hipMemcpyDeviceToHost, stream_));
    PHX_HIP(hipStreamSynchronize(stream_));
    de.release();
    ds.release();
    return PHX_OK;
}

int DeviceBroadphase::erase_pairs_device(const uint2* d_pairs, int count)
{
    PHX_TRY(use_device(device_));
    PHX_REQUIRE(count >= 0 && (count == 0 || d_pairs), "bad pair list");
    if (!count) return PHX_OK;
    hipLaunchKernelGGL(k_ps_erase, dim3(grid_for(count)), dim3(256), 0, stream_, table_.p, table_cap_ - 1, d_pairs, count, erase_count_.p);
    PHX_HIP(hipGetLastError());
    // Booked as if every pair was found (a World only erases pairs it inserted); the device counter says how many really
    // were, and the difference is settled with the next readback this handle makes anyway (reconcile_erases) — an erase
    // costs no host round trip of its own.  set_size_ + tombstones_, which sizes the table, is right either way.
    set_size_ -= count;
    tombstones_ += count;
    erase_unchecked_ += count;
    return PHX_OK;
}

// the pair set of a restored world (World::set_state): one pair per live manifold, as the broadphase would hold it (ref: Collider.h:58
// manifoldMap is keyed by the manifold's ordered body pair)
int DeviceBroadphase::reset_pairs(const uint2* pairs, int count)
{
    PHX_TRY(stage_pairs(pairs, count));
    PHX_TRY(reset_pairs_device(scratch_pairs_.p, count));
    PHX_HIP(hipStreamSynchronize(stream_));          // (`pairs` is the caller's)
    return PHX_OK;
}

// the same from pairs already in HBM (a World's removal of bodies: the kept manifolds' pairs), queued on the stream
int DeviceBroadphase::reset_pairs_device(const uint2* d_pairs, int count)
{
    PHX_TRY(use_device(device_));
    PHX_REQUIRE(count >= 0 && (count == 0 || d_pairs), "bad pair list");
    PHX_TRY(clear());
    have_update_ = false;
    if (!count) return PHX_OK;
    PHX_TRY(resize_table(4u * (unsigned)count + 1024u));
    hipLaunchKernelGGL(k_ps_insert, dim3(grid_for(count)), dim3(256), 0, stream_, table_.p, table_cap_ - 1, d_pairs, count, (unsigned long long*)nullptr);
    PHX_HIP(hipGetLastError());
    set_size_ = count;
    stats_.set_size = count;
    return PHX_OK;
}

int pair_table_fill(unsigned long long* table, unsigned cap, const uint2* d_pairs, int n, hipStream_t stream)
{
    PHX_REQUIRE(table && cap && !(cap & (cap - 1u)) && n >= 0 && (unsigned)n <= cap / 2u, "bad pair table");
    PHX_HIP(hipMemsetAsync(table, 0xFF, (size_t)cap * sizeof(unsigned long long), stream));
    if (n) hipLaunchKernelGGL(k_ps_insert, dim3(grid_for(n)), dim3(256), 0, stream, table, cap - 1u, d_pairs, n, (unsigned long long*)nullptr);
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

// queue the read of the device's erase counter with a batch the caller is about to wait for ...
int DeviceBroadphase::queue_erase_check(int* erased)
{
    *erased = 0;
    if (!erase_unchecked_) return PHX_OK;
    return rb_.add(erased, erase_count_.p, sizeof(int), stream_);
}

// ... and settle the books afterwards
int DeviceBroadphase::settle_erase_check(int erased)
{
    if (!erase_unchecked_) return PHX_OK;
    const long long missing = erase_unchecked_ - erased;             // requested pairs that were not in the set
    set_size_ += missing;
    tombstones_ = std::max<long long>(0, tombstones_ - missing);
    erase_unchecked_ = 0;
    PHX_HIP(hipMemsetAsync(erase_count_.p, 0, sizeof(int), stream_));
    return PHX_OK;
}

// a host pair list (`count` x 2 body indices), checked and queued into scratch_pairs_
int DeviceBroadphase::stage_pairs(const void* pairs, int count)
{
    PHX_TRY(use_device(device_));
    PHX_REQUIRE(count >= 0 && (count == 0 || pairs), "bad pair list");
    if (!count) return PHX_OK;
    PHX_TRY(scratch_pairs_.reserve((size_t)count));
    PHX_HIP(hipMemcpyAsync(scratch_pairs_.p, pairs, (size_t)count * sizeof(uint2), hipMemcpyHostToDevice, stream_));
    return PHX_OK;
}

int DeviceBroadphase::erase_pairs(const uint32_t* pairs, int count)
{
    PHX_TRY(stage_pairs(pairs, count));
    return erase_pairs_device(scratch_pairs_.p, count);      // (nothing to do for an empty list)
}

int DeviceBroadphase::get_stats(phx_broadphase_stats* out)
{
    PHX_REQUIRE(out, "null out");
    PHX_TRY(require_update());
    PHX_TRY(use_device(device_));
    if (ms_pending_) {
        unsigned long long stamps[2] = {0, 0};
        PHX_TRY(rb_.add(stamps, stamps_.p, sizeof stamps, stream_));
        PHX_TRY(rb_.wait(stream_));
        stats_.device_ms = stamps[1] > stamps[0] ? (double)(stamps[1] - stamps[0]) * 1e-5 : 0.0;      // 100 MHz ticks -> ms
        ms_pending_ = false;
    }
    if (erase_unchecked_) {
        int erased = 0;
        PHX_TRY(queue_erase_check(&erased));
        PHX_TRY(rb_.wait(stream_));
        PHX_TRY(settle_erase_check(erased));
    }
    *out = stats_;
    out->set_size = (int)set_size_;
    return PHX_OK;
}

} // namespace phx
