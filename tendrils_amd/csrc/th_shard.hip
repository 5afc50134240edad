// th_shard.hip - row-band shards: the draw() exchange (emit by owner, merge, th_draw_sharded), the job's
// communicator, the particle-texture gather of the spawners, the counter all-reduce, the sampled spawn that fetches its taps.
#include "th_ctx.hpp"

using namespace thi;

namespace thi {

th_status texels_fit_keys(const th_context *c, const char *target)
{
    TH_REQUIRE((uint64_t)c->fw * c->fh <= (uint64_t)th::kTexelMask + 1u, "the sharded deposit keys hold 24 texel bits: %s %dx%d is too large", target, c->fw, c->fh);
    return TH_OK;
}

// the tail of every emit: the fragments of the (prepared) pass `p` - this band's lines - counted, scanned, keyed (owner,
// texel, global stream index), handed to the pass's fragment stage if it has one, and parted by owner
th_status emit_parted(th_context *c, th::DepositParams &p, const FragmentStage *stage, uint64_t *count, void **keys_dev, void **colors_dev)
{
    th::launch_deposit_count(p, c->stream);
    uint32_t total = 0;
    if (th_status s = deposit_scan_total(c, p, &total)) return s;
    *count = total; *keys_dev = nullptr; *colors_dev = nullptr;
    if (total == 0) return TH_OK;
    const bool pairs = p.mode == 2;                  // th_draw_emit: two varyings per fragment, side by side
    if (th_status s = deposit_reserve(c, total, true, pairs, stage_reads_line(stage))) return s;
    p.keys64 = c->dep_u64[0]; p.slots = c->dep_u32[1]; p.colors = c->dep_colors;
    p.owners = c->dep_owners;
    p.owner_chunk = (uint32_t)(((uint64_t)c->fw * c->fh + p.owners - 1u) / p.owners);
    th::launch_deposit_scatter(p, c->stream);
    // (a caller's fragment stage, th_draw_stages_emit: here keys64[i] and colors[i] still name the same fragment)
    if (stage) if (th_status s = fragment_stage_run(c, *stage, p, total)) return s;
    *keys_dev = c->dep_u64[0]; *colors_dev = c->dep_colors;
    if (p.owners > 1u) {
        // the fragment array is in this band's stream order: ONE stable pass on the owner bits parts it by destination
        // (every part still in stream order); the owners sort by texel
        int owner_bits = 1;
        while ((1u << owner_bits) < p.owners) ++owner_bits;
        if (th_status s = deposit_temp(c, th::radix_sort_temp_bytes(total, th::kOwnerShift, th::kOwnerShift + owner_bits))) return s;
        const int in_b = th::launch_radix_sort_u64(c->dep_u64[0], c->dep_u32[1], c->dep_u64[1], c->dep_u32[3], total, th::kOwnerShift,
                                                   th::kOwnerShift + owner_bits, c->dep_temp, true, c->stream);
        if (pairs) th::launch_deposit_gather_pairs(c->dep_colors_sorted, c->dep_colors, in_b ? c->dep_u32[3] : c->dep_u32[1], total, c->stream);
        else th::launch_deposit_gather_colors(c->dep_colors_sorted, c->dep_colors, in_b ? c->dep_u32[3] : c->dep_u32[1], total, c->stream);
        *keys_dev = in_b ? c->dep_u64[1] : c->dep_u64[0]; *colors_dev = c->dep_colors_sorted;
    }
    TH_HIP(hipGetLastError());
    TH_HIP(hipStreamSynchronize(c->stream));               // the caller hands the buffers to a collective on its own stream
    return TH_OK;
}

}  // namespace thi

extern "C" {

th_status th_deposit_set_owners(th_context *c, int32_t world)
{
    TH_REQUIRE(c, "null context");
    // (the owner's merge walks up to 32 source bands per texel - th_deposit.hip: kMaxBands: more ranks than that could only be
    // refused after the blend had begun)
    TH_REQUIRE(world >= 1 && world <= 32, "owner count %d outside [1, 32]", world);
    c->dep_owners = (uint32_t)world;
    return TH_OK;
}

th_status th_deposit_emit(th_context *c, const th_deposit_uniforms *u, uint64_t *count, void **keys_dev, void **colors_dev)
{
    if (th_status s = use(c)) return s;
    TH_REQUIRE(count && keys_dev && colors_dev, "null outputs");
    return pass_emit(c, builtin_pass(TH_PASS_FLOW, u), count, keys_dev, colors_dev);
}

// the view pass of a row-band shard: the same lines with the render shader's colours
th_status th_view_emit(th_context *c, const th_render_uniforms *u, uint64_t *count, void **keys_dev, void **colors_dev)
{
    if (th_status s = use(c)) return s;
    TH_REQUIRE(count && keys_dev && colors_dev, "null outputs");
    return pass_emit(c, builtin_pass(TH_PASS_VIEW, u), count, keys_dev, colors_dev);
}

// both passes of a row-band shard's draw() in one: every fragment with the flow pass's varying and the view pass's colour
// side by side (32 bytes), rasterised, parted and - by the host or th_draw_sharded - exchanged once
static th_status draw_emit(th_context *c, const th_deposit_uniforms *du, const th_render_uniforms *ru, uint64_t *count, void **keys_dev, void **colors_dev)
{
    TH_REQUIRE(du && ru && count && keys_dev && colors_dev, "null argument");
    if (th_status s = texels_fit_keys(c, "target")) return s;
    if (th_status s = shared_uniforms(du, ru)) return s;
    TH_REQUIRE(drawn_line_width(c, TH_PASS_FLOW) == drawn_line_width(c, TH_PASS_VIEW),
               "the two passes draw their lines %g and %g wide: th_deposit_emit and th_view_emit rasterise them apart",
               (double)drawn_line_width(c, TH_PASS_FLOW), (double)drawn_line_width(c, TH_PASS_VIEW));
    th::DepositParams p;
    if (th_status s = deposit_prepare(c, du, p)) return s;
    p.mode = 2;
    view_fields(c, ru, p);
    return emit_parted(c, p, nullptr, count, keys_dev, colors_dev);
}

th_status th_draw_emit(th_context *c, const th_deposit_uniforms *du, const th_render_uniforms *ru, uint64_t *count, void **keys_dev, void **colors_dev)
{
    if (th_status s = use(c)) return s;
    return draw_emit(c, du, ru, count, keys_dev, colors_dev);
}

th_status th_deposit_set_halo(th_context *c, const void *lo_dev, const void *hi_dev)
{
    TH_REQUIRE(c, "null context");
    c->halo_lo = static_cast<const float4 *>(lo_dev);
    c->halo_hi = static_cast<const float4 *>(hi_dev);
    return TH_OK;
}

static th_status merge_reserve(th_context *c, uint32_t total, int target);

// target: 0 = the flow texture, 1 = the view buffer, 2 = both (the fragments carry pairs of varyings: th_draw_emit)
static th_status merge_parted(th_context *c, const void *keys_dev, const void *colors_dev, uint64_t count, int target)
{
    if (count == 0) return TH_OK;
    TH_REQUIRE(keys_dev && colors_dev && count < (1ull << 31), "bad fragment buffers");
    const uint32_t total = (uint32_t)count;
    if (th_status s = merge_reserve(c, total, target)) return s;
    // what arrives is one part per source band, every part in that band's stream order: a stable sort by texel (the
    // owner bits above and the stream index below are left alone), then the blend merges the bands inside each texel
    const int bits = 32 + deposit_texel_bits(c);
    TH_HIP(hipMemsetAsync(c->dep_total, 0, 8 * sizeof(uint32_t), c->stream));
    // (the sort ping-pongs between its two buffer pairs: the caller's keys are copied, not sorted in place)
    TH_HIP(hipMemcpyAsync(c->mrg_keys, keys_dev, (size_t)total * sizeof(unsigned long long), hipMemcpyDeviceToDevice, c->stream));
    const int in_b = th::launch_radix_sort_u64(c->mrg_keys, c->mrg_vals[0], c->mrg_keys2, c->mrg_vals[1], total, 32, bits, c->dep_temp, true, c->stream);
    const unsigned long long *keys = in_b ? c->mrg_keys2 : c->mrg_keys;          // (the pair the sort ended in)
    const uint32_t *vals = in_b ? c->mrg_vals[1] : c->mrg_vals[0];
    const float4 *colors = static_cast<const float4 *>(colors_dev);
    if (target == 2) th::launch_draw_blend64(c->flow, c->view, keys, vals, colors, c->mrg_colors, total, c->dep_total, c->stream);
    else if (target == 1) th::launch_view_blend64(c->view, keys, vals, colors, c->mrg_colors, total, c->dep_total, c->stream);
    else th::launch_deposit_blend64(c->flow, keys, vals, colors, c->mrg_colors, total, c->dep_total, c->stream);
    TH_HIP(hipGetLastError());
    uint32_t too_many = 0;
    if (th_status s = read_back(c, &too_many, c->dep_total, sizeof too_many)) return s;        // (a sync: the input buffers may be reused by the caller now)
    if (too_many) return fail(TH_ERR_UNSUPPORTED, "a texel received fragments of more than 32 source bands");
    return TH_OK;
}

// ... as the three entry points and th_draw_sharded's passes go about it: a merge into the view buffer writes no state and no flow
static th_status merge_pass(th_context *c, const void *keys_dev, const void *colors_dev, uint64_t count, int target)
{
    if (th_status s = use(c, target != 0)) return s;
    if (target != 0) if (th_status s = view_storage(c)) return s;
    return merge_parted(c, keys_dev, colors_dev, count, target);
}

th_status th_deposit_merge(th_context *c, const void *keys_dev, const void *colors_dev, uint64_t count) { return merge_pass(c, keys_dev, colors_dev, count, 0); }
th_status th_view_merge(th_context *c, const void *keys_dev, const void *colors_dev, uint64_t count) { return merge_pass(c, keys_dev, colors_dev, count, 1); }
th_status th_draw_merge(th_context *c, const void *keys_dev, const void *colors_dev, uint64_t count) { return merge_pass(c, keys_dev, colors_dev, count, 2); }

// ---- draw() of a row-band shard, the exchange issued by the library over its own communicator ---------------------------------
// A rank that fails on its own (a line that needs a halo row nobody supplied, an allocation) must not leave the others
// waiting inside a collective: before every exchange whose size or success depends on something rank-local, the ranks
// agree on a status word, and all of them leave together.
constexpr unsigned long long kPeerFailed = 1ull << 62;       // (a count travels below bit 31)
constexpr unsigned long long kPeerRetries = 1ull << 61;      // ... a rank whose binned pass gave up: everybody takes the stream-ordered pass

// (TH_TESTING builds: TH_OPT_INJECT_FAILURE) this rank fails at `stage` once; a release build has no such switch
#ifdef TH_TESTING
static th_status injected(th_context *c, int stage)
{
    if (c->opt.inject_failure != stage) return TH_OK;
    c->opt.inject_failure = 0;
    return fail(TH_ERR_UNSUPPORTED, "injected failure at stage %d of the sharded draw (TH_OPT_INJECT_FAILURE)", stage);
}
static bool injected_give_up(th_context *c)       // value 4: this rank's binned pass gives up (everybody takes the stream-ordered pass)
{
    if (c->opt.inject_failure != 4) return false;
    c->opt.inject_failure = 0;
    return true;
}
#else
static th_status injected(th_context *, int) { return TH_OK; }
static bool injected_give_up(th_context *) { return false; }
#endif

static th_status peer_failure(th_context *c, int who, const char *stage, bool spawn = false)
{
    if (spawn) return fail(TH_ERR_UNSUPPORTED, "sharded spawn: rank %d failed while %s (this rank, %d, had no error of its own)", who, stage, c->comm_rank);
    return fail(TH_ERR_UNSUPPORTED, "sharded draw: rank %d failed while %s (this rank, %d, had no error of its own); nothing was blended", who, stage, c->comm_rank);
}

// every rank hands in its status; all of them return TH_OK, or none does (a failing rank returns its own error)
static th_status agree_status(th_context *c, th_status mine, const char *stage, bool spawn = false)
{
    if (c->comm_world <= 1) return mine;
    const std::string why = mine != TH_OK ? last_error() : std::string();
    // the lowest failing rank wins the maximum; a failure (2) outranks a binned pass that only wants the stream-ordered pass (1)
    const uint32_t word = mine != TH_OK ? (((uint32_t)(c->comm_world - c->comm_rank)) | (mine == kRetryInStreamOrder ? 0x10000u : 0x20000u)) : 0u;
    th::launch_exchange_word(c->d_status, word, c->stream);         // (from the kernel arguments: no host buffer to outlive, no sync)
    const hipError_t e = hipGetLastError();
    if (c->transport->allreduce_max_u32(c->comm, c->d_status, c->stream)) return fail(TH_ERR_UNSUPPORTED, "%s", th::comm_error());
    uint32_t worst = 0;
    if (th_status s = read_back(c, &worst, c->d_status, sizeof worst)) return s;
    TH_HIP(e);
    if ((worst >> 16) == 1u) return kRetryInStreamOrder;              // (every rank returns this together)
    if (mine != TH_OK) { last_error() = why; return mine; }
    if (worst) return peer_failure(c, c->comm_world - (int)(worst & 0xffffu), stage, spawn);
    return TH_OK;
}

// scratch of the owner's merge for `total` received fragments (grow-only); target 2: room for two varyings per fragment
static th_status merge_reserve(th_context *c, uint32_t total, int target)
{
    if (target == 2 && !c->mrg_pairs) {
        c->mrg_pairs = true;
        if (c->mrg_capacity) if (th_status s = c->mrg_colors.alloc(2 * c->mrg_capacity)) { c->mrg_capacity = 0; return s; }
    }
    if (c->mrg_capacity < total) {
        c->mrg_keys.reset(); c->mrg_keys2.reset(); c->mrg_vals[0].reset(); c->mrg_vals[1].reset(); c->mrg_colors.reset(); c->mrg_capacity = 0;
        const size_t cap = (size_t)total + (size_t)total / 4 + 1024;
        if (th_status s = c->mrg_keys.alloc(cap)) return s;
        if (th_status s = c->mrg_keys2.alloc(cap)) return s;
        if (th_status s = c->mrg_vals[0].alloc(cap)) return s;
        if (th_status s = c->mrg_vals[1].alloc(cap)) return s;
        if (th_status s = c->mrg_colors.alloc((c->mrg_pairs ? 2 : 1) * cap)) return s;
        c->mrg_capacity = cap;
    }
    if (th_status s = deposit_temp(c, th::radix_sort_temp_bytes(total, 32, 32 + deposit_texel_bits(c)))) return s;
    return c->dep_total.reserve(th::kTotWords, th::kTotWords);
}

// room for `total` received fragments (grow-only; both: two varyings each).  x_keys.size() is the capacity: the keys are
// allocated last, so that they are only there when the varyings are
static th_status exchange_room(th_context *c, size_t total, bool both)
{
    if (c->x_keys.size() >= total && (c->x_pairs || !both)) return TH_OK;
    const size_t cap = std::max(total, c->x_keys.size()) + total / 4 + 1024;
    c->x_keys.reset(); c->x_colors.reset();
    c->x_pairs = c->x_pairs || both;
    if (th_status s = c->x_colors.alloc((c->x_pairs ? 2 : 1) * cap)) return s;
    return c->x_keys.alloc(cap);
}

// the owners' ranges [lo[r], hi[r]) - in texels - of the target(s) a pass drew to every rank, in place
static th_status gather_owned(th_context *c, bool view, bool both, const std::vector<size_t> &lo, const std::vector<size_t> &hi)
{
    const int world = c->comm_world, rank = c->comm_rank;
    for (int plane_of = 0; plane_of < 2; ++plane_of) {          // 0: the flow texture, 1: the view buffer
        if (plane_of == 0 ? (view && !both) : !view) continue;
        const size_t elem = plane_of ? sizeof(uchar4) : sizeof(float4);
        std::vector<size_t> gb((size_t)world), go((size_t)world);
        for (int r = 0; r < world; ++r) { gb[(size_t)r] = (hi[(size_t)r] - lo[(size_t)r]) * elem; go[(size_t)r] = lo[(size_t)r] * elem; }
        char *plane = plane_of ? reinterpret_cast<char *>(c->view) : reinterpret_cast<char *>(c->flow.get());
        if (c->transport->allgather_bytes(c->comm, plane + go[(size_t)rank], plane, gb.data(), go.data(), rank, world, c->stream))
            return fail(TH_ERR_UNSUPPORTED, "%s", th::comm_error());
        for (int r = 0; r < world; ++r) if (r != rank) c->last_draw.received_bytes += gb[(size_t)r];
        if (world > 1) c->last_draw.sent_bytes += gb[(size_t)rank];
    }
    return TH_OK;
}

// ---- the count exchange -----------------------------------------------------------------------------------------------------
// x_counts, on the device: the owners' bounds of what this rank holds (world + 1 words, world <= 32), what it holds for every
// owner, what every rank holds for it.  (The bounds stay on the device: what this rank holds for every owner is their
// differences, computed there, and comes back to the host together with what the others hold for it - one trip where there
// were two.  A rank with something to report, or nothing to send, uploads its words itself.)
constexpr size_t kXBounds = 0, kXSend = 33, kXRecv = 65, kXWords = 97;
struct CountExchange {
    std::vector<size_t> scount, soff, rcount, roff;      // fragments for / from every rank, and where each rank's part begins
    size_t total = 0;                                    // ... received in all
};

// One word per rank each way.  `mine`: how this rank's stage 1 went - whether it worked travels with the counts, so every rank
// learns of every failure (kPeerFailed) and of a binned pass that gave up (kPeerRetries: nobody sends it in the stream-ordered
// pass, and no count reaches bit 32 there); on_device: this rank's counts are at kXSend already.  A rank that failed returns its
// own error; kRetryInStreamOrder on every rank together.
static th_status exchange_counts(th_context *c, th_status mine, bool on_device, CountExchange &x)
{
    const size_t world = (size_t)c->comm_world;
    unsigned long long *sendc = c->x_counts + kXSend, *recvc = c->x_counts + kXRecv;
    const std::string why = mine != TH_OK ? last_error() : std::string();
    std::vector<size_t> one(world, 1), idx(world);
    for (size_t r = 0; r < world; ++r) idx[r] = r;
    const std::vector<unsigned long long> hs(world, mine == TH_OK ? 0ull : (mine == kRetryInStreamOrder ? kPeerRetries : kPeerFailed));
    if (!on_device) TH_HIP(hipMemcpyAsync(sendc, hs.data(), world * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
    if (c->transport->alltoallv(c->comm, sendc, one.data(), idx.data(), recvc, one.data(), idx.data(), sizeof(unsigned long long), (int)world, c->stream))
        return fail(TH_ERR_UNSUPPORTED, "%s", th::comm_error());
    std::vector<unsigned long long> words(kXWords);
    if (th_status s = read_back(c, words.data(), c->x_counts, words.size() * sizeof(unsigned long long))) return s;
    const unsigned long long *hb = words.data() + kXBounds, *hr = words.data() + kXRecv;
    x.scount.assign(world, 0); x.soff.assign(world, 0); x.rcount.assign(world, 0); x.roff.assign(world, 0);
    if (on_device) for (size_t r = 0; r < world; ++r) { x.scount[r] = (size_t)(hb[r + 1] - hb[r]); x.soff[r] = (size_t)hb[r]; }
    if (mine != TH_OK && mine != kRetryInStreamOrder) { last_error() = why; return mine; }
    for (size_t r = 0; r < world; ++r) if (hr[r] & kPeerFailed) return peer_failure(c, (int)r, "rasterising its band's lines");
    for (size_t r = 0; r < world; ++r) if (hr[r] & kPeerRetries) return kRetryInStreamOrder;
    x.total = 0;
    for (size_t r = 0; r < world; ++r) { x.rcount[r] = (size_t)(hr[r] & 0xffffffffull); x.roff[r] = x.total; x.total += x.rcount[r]; }
    return TH_OK;
}

// the fragments change hands: the keys, then the varyings, as the counts said
static th_status exchange_fragments(th_context *c, const void *keys, const void *colors, size_t color_bytes, const CountExchange &x)
{
    const int world = c->comm_world;
    if (c->transport->alltoallv(c->comm, keys, x.scount.data(), x.soff.data(), c->x_keys, x.rcount.data(), x.roff.data(), sizeof(unsigned long long), world, c->stream) ||
        c->transport->alltoallv(c->comm, colors, x.scount.data(), x.soff.data(), c->x_colors, x.rcount.data(), x.roff.data(), color_bytes, world, c->stream))
        return fail(TH_ERR_UNSUPPORTED, "%s", th::comm_error());
    return TH_OK;
}

// One pass: this band's fragments parted by owner -> all-to-all -> the owner's merge -> all-gather of the owned ranges.
// spec: the flow pass or the view pass, with the built-in vertex stage or a draw program's; null: both passes with the built-in stages of du and ru
// over one rasterisation and one exchange (two all-gathers).  Whatever fails inside the emit (stage 1) fails on this rank alone, and travels with the counts
static th_status sharded_pass(th_context *c, const PassSpec *spec, const th_deposit_uniforms *du, const th_render_uniforms *ru, uint64_t *fragments)
{
    const bool both = !spec, view = both || spec->pass == TH_PASS_VIEW;
    const int world = c->comm_world, rank = c->comm_rank;
    const size_t color_bytes = both ? 2 * sizeof(float4) : sizeof(float4);
    uint64_t count = 0;
    void *keys = nullptr, *colors = nullptr;
    // stage 1 - rasterise and part by owner
    th_status mine = injected(c, 2);
    if (mine == TH_OK) mine = both ? draw_emit(c, du, ru, &count, &keys, &colors) : pass_emit(c, *spec, &count, &keys, &colors);
    // (exchange_counts would pass kRetryInStreamOrder on as a wish for this very pass: no emit returns it, and if one ever did it is a failure here)
    if (mine == kRetryInStreamOrder) mine = fail(TH_ERR_HIP, "the stream-ordered emit asked for the stream-ordered pass");
    if (fragments) *fragments = mine == TH_OK ? count : 0;
    draw_streamed(c, mine == TH_OK ? count : 0);
    const bool on_device = mine == TH_OK && count;
    if (on_device) {
        th::launch_owner_bounds(static_cast<const unsigned long long *>(keys), (uint32_t)count, (uint32_t)world, c->x_counts + kXBounds, c->stream);
        th::launch_exchange_send_counts(c->x_counts + kXBounds, (uint32_t)world, c->x_counts + kXSend, c->stream);
        TH_HIP(hipGetLastError());
    }
    CountExchange x;
    if (th_status s = exchange_counts(c, mine, on_device, x)) return s;
    for (int r = 0; r < world; ++r) if (r != rank) {
        c->last_draw.sent_bytes += 8 + x.scount[(size_t)r] * (sizeof(unsigned long long) + color_bytes);
        c->last_draw.received_bytes += 8 + x.rcount[(size_t)r] * (sizeof(unsigned long long) + color_bytes);
    }
    // stage 2 - room for what arrives and for its merge: the last thing that can fail on one rank alone
    const size_t total = x.total;
    mine = total < ((size_t)1 << 31) ? TH_OK : fail(TH_ERR_UNSUPPORTED, "too many fragments for one owner");
    auto room = [&]() -> th_status {
        if (th_status s = exchange_room(c, total, both)) return s;
        return merge_reserve(c, (uint32_t)total, both ? 2 : (view ? 1 : 0));
    };
    if (mine == TH_OK) mine = injected(c, 3);
    if (mine == TH_OK) mine = room();
    if (th_status s = agree_status(c, mine, "making room for the fragments it owns")) return s;
    // stage 3 - the exchange, the merge, the owned ranges back to everybody
    if (th_status s = exchange_fragments(c, keys, colors, color_bytes, x)) return s;
    if (th_status s = merge_pass(c, c->x_keys, c->x_colors, total, both ? 2 : (view ? 1 : 0))) return s;
    // the owners' texel ranges of the target(s) to every rank, in place
    const size_t texels = (size_t)c->fw * c->fh, chunk = (texels + (size_t)world - 1) / (size_t)world;
    std::vector<size_t> lo((size_t)world), hi((size_t)world);
    for (int r = 0; r < world; ++r) { lo[(size_t)r] = std::min(texels, (size_t)r * chunk); hi[(size_t)r] = std::min(texels, ((size_t)r + 1) * chunk); }
    return gather_owned(c, view, both, lo, hi);
}

// ---- the same pass through the BINS, in its parts ------------------------------------------------------------------------------
// the owner's tables inside own_mem (grow-only): the 8-byte arrays first
static th_status owner_tables(th_context *c, const th::DepositParams &p, th::OwnerParams &o)
{
    const size_t words = (size_t)p.nbins * (1 + 2 + 1 + 1 + 32 * 1 + 32 * 2) + 2 * (2 + 33 + 32) + 64;
    if (c->own_mem.size() < words) {
        TH_HIP(hipStreamSynchronize(c->stream));
        if (th_status s = c->own_mem.alloc(words)) return s;
    }
    unsigned long long *q = reinterpret_cast<unsigned long long *>(c->own_mem.get());
    o.offsets = q; q += (size_t)p.nbins + 1;
    q += 33;                                               // (the owners' bounds lived here: they lie beside the counts now)
    o.owner_bounds = c->x_counts + kXBounds;
    o.recv_base = q; q += 32;
    o.src_prefix = q; q += (size_t)32 * p.nbins;
    uint32_t *w = reinterpret_cast<uint32_t *>(q);
    o.counts = w; w += p.nbins;
    o.bin_total = w; w += p.nbins;
    o.bin_page = w; w += p.nbins;
    o.table = w;
    return TH_OK;
}

// stage 1: my band's lines into my store, then compacted owner by owner; the counts for every owner are left on the device
// (the owners' bounds come back with the counts the others send: one trip, exchange_counts)
static th_status bins_emit_by_owner(th_context *c, const th_deposit_uniforms *du, const th_render_uniforms *ru, th::DepositParams &p, th::OwnerParams &o, uint32_t *emitted)
{
    const int world = c->comm_world, rank = c->comm_rank;
    const bool view = ru != nullptr, both = ru != nullptr && du != nullptr;
    const th_deposit_uniforms d = du ? *du : deposit_uniforms_of(*ru);
    if (th_status s = injected(c, 2)) return s;
    if (injected_give_up(c)) return kRetryInStreamOrder;
    if (th_status s = deposit_prepare_bins(c, &d, p)) return s;
    p.mode = both ? 2 : (view ? 1 : 0);
    if (view) { view_fields(c, ru, p); p.view = c->view; if (!both) p.line_half = 0.5f * drawn_line_width(c, TH_PASS_VIEW); }
    if (th_status s = bins_pass_emit(c, p, false)) return s;
    const uint32_t *host = c->bins_totals_host;
    o.pool_used = host[th::kTotPool];                     // (my own bins stay in the store: what arrives goes behind them)
    *emitted = host[th::kTotFragments];
    const uint32_t bins_y = p.nbins / p.bins_x;
    o.world = (uint32_t)world; o.rank = (uint32_t)rank;
    for (int r = 0; r <= world; ++r) o.bin_lo[r] = (uint32_t)((unsigned long long)bins_y * (unsigned)r / (unsigned)world) * p.bins_x;
    o.nb = o.bin_lo[rank + 1] - o.bin_lo[rank];
    if (th_status s = owner_tables(c, p, o)) return s;
    const uint32_t total = *emitted;                       // (an upper bound of what leaves)
    if (total) {
        if (th_status s = deposit_reserve(c, total, true, both)) return s;
        o.out_keys = c->dep_u64[0]; o.out_colors = c->dep_colors;
    }
    th::launch_bins_owner_counts(p, o, c->stream);
    if (total) th::launch_bins_owner_extract(p, o, c->stream);
    th::launch_exchange_send_counts(o.owner_bounds, (uint32_t)world, c->x_counts + kXSend, c->stream);
    TH_HIP(hipGetLastError());
    return TH_OK;
}

// stage 3, the layout: the received bins into the owner's store as if it had emitted them, repeated with a wider table / a
// larger pool that KEEP what the store holds.  `laid`: how it went - the ranks agree on it; what is returned otherwise ends the
// call at once, as a failing launch or read-back does anywhere
static th_status owner_lay_out(th_context *c, th::DepositParams &p, const th::OwnerParams &o, th_status *laid)
{
    const uint32_t *host = c->bins_totals_host;
    for (int attempt = 0;; ++attempt) {
        TH_HIP(hipMemsetAsync(c->dep_total, 0, th::kTotWords * sizeof(uint32_t), c->stream));
        bins_pass_expect(c, p);
        th::launch_bins_owner_insert(p, o, c->stream);
        TH_HIP(hipGetLastError());
        if (th_status s = bins_pass_totals(c, p)) return s;
        const uint32_t flags = host[th::kTotFlags];
        if (flags == 0) return TH_OK;
        // (nothing has been blended; a bin beyond its lists' reach cannot be drawn through the bins at all)
        if (bins_flags_final(flags, attempt)) { *laid = fail(TH_ERR_UNSUPPORTED, "the bins this rank owns could not be laid out (flags %u)", flags); return TH_OK; }
        if (flags & th::kBinsBinFull) {         // (a wider page table, with the entries of what this rank emitted itself)
            if ((*laid = bins_table_widen(c, p, true)) == kRetryInStreamOrder)
                *laid = fail(TH_ERR_UNSUPPORTED, "a bin of the target received more fragments than its lists hold (%u places)", c->bin_max_pages * th::kBinPage * th::kBinReplicas);
            if (*laid != TH_OK) return TH_OK;
        }
        if ((flags & th::kBinsPoolExhausted) && (*laid = bins_store_grow_keep(c, p, host[th::kTotPool] + host[th::kTotPool] / 2u + 64u)) != TH_OK) return TH_OK;
    }
}

// The same pass through the BINS (th_bins.hip "the bins travel to the ranks that own them"): every rank rasterises its band's
// lines into its own page store over whatever slot order its ring is held in (the integrator's tile-sorted one: no return to
// texel order, no 64-bit keys, no sort anywhere); an owner owns whole bin rows; the bins change hands bin by bin with their
// counts beside them and are laid out in the owner's store as if it had emitted them; plan and blend kernels as in a single
// context.  kRetryInStreamOrder (on every rank together): a store could not be had or a bin outgrew its lists - the caller
// runs the stream-ordered pass.  (last_draw.pipeline is bins_pass_finish's to set: a pass that ends before it reports nothing.)
static th_status sharded_pass_bins(th_context *c, const th_deposit_uniforms *du, const th_render_uniforms *ru, uint64_t *fragments)
{
    const int world = c->comm_world, rank = c->comm_rank;
    const bool view = ru != nullptr, both = ru != nullptr && du != nullptr;
    const size_t color_bytes = both ? 2 * sizeof(float4) : sizeof(float4);
    // ---- stage 1: my band's lines into my store, then compacted owner by owner
    th::DepositParams p;
    th::OwnerParams o{};
    uint32_t emitted = 0;
    th_status mine = bins_emit_by_owner(c, du, ru, p, o, &emitted);
    if (fragments) *fragments = mine == TH_OK ? emitted : 0;          // (what leaves + what stays)
    CountExchange x;
    if (th_status s = exchange_counts(c, mine, mine == TH_OK, x)) return s;
    // (counts word, the per-bin counts of the owner's bins, keys + varyings of what changes hands)
    for (int r = 0; r < world; ++r) if (r != rank) {
        c->last_draw.sent_bytes += 8 + (size_t)(o.bin_lo[r + 1] - o.bin_lo[r]) * sizeof(uint32_t) + x.scount[(size_t)r] * (sizeof(unsigned long long) + color_bytes);
        c->last_draw.received_bytes += 8 + (size_t)o.nb * sizeof(uint32_t) + x.rcount[(size_t)r] * (sizeof(unsigned long long) + color_bytes);
    }
    // ---- stage 2: every source's counts for my bins; room for what arrives; my store laid out for it (the last things that can
    // fail on one rank alone: agreed on before the fragments travel)
    {
        std::vector<size_t> tc((size_t)world), to((size_t)world), rc((size_t)world, o.nb), ro((size_t)world);
        for (int r = 0; r < world; ++r) { tc[(size_t)r] = o.bin_lo[r + 1] - o.bin_lo[r]; to[(size_t)r] = o.bin_lo[r]; ro[(size_t)r] = (size_t)r * o.nb; }
        if (c->transport->alltoallv(c->comm, o.counts, tc.data(), to.data(), const_cast<uint32_t *>(o.table), rc.data(), ro.data(), sizeof(uint32_t), world, c->stream))
            return fail(TH_ERR_UNSUPPORTED, "%s", th::comm_error());
    }
    auto stage2 = [&]() -> th_status {
        if (th_status s = injected(c, 3)) return s;
        if (x.total >= ((size_t)1 << 31)) return fail(TH_ERR_UNSUPPORTED, "too many fragments for one owner");
        if (world > 1) if (th_status s = exchange_room(c, x.total, both)) return s;
        // (where every source's part starts in what arrives: the running sum of the received counts, made on the device)
        th::launch_exchange_recv_base(c->x_counts + kXRecv, (uint32_t)world, const_cast<unsigned long long *>(o.recv_base), c->stream);
        TH_HIP(hipGetLastError());
        return TH_OK;
    };
    mine = stage2();
    if (th_status s = agree_status(c, mine, "making room for the bins it owns")) return s;
    // ---- stage 3: the bins travel; laid out and blended where they are owned; the owned rows back to everybody
    if (world == 1) { o.in_keys = o.out_keys; o.in_colors = o.out_colors; }        // (nobody to send to: the compacted parts are the received ones)
    else {
        if (th_status s = exchange_fragments(c, o.out_keys, o.out_colors, color_bytes, x)) return s;
        o.in_keys = c->x_keys; o.in_colors = c->x_colors;
    }
    th_status laid = TH_OK;
    if (th_status s = owner_lay_out(c, p, o, &laid)) return s;
    if (laid == TH_OK) laid = bins_pass_finish(c, p, nullptr, false);
    // (an owner that could not lay its bins out has blended nothing; the others have: the draw is lost, and everybody says so)
    if (th_status s = agree_status(c, laid == kRetryInStreamOrder ? fail(TH_ERR_HIP, "the owner's store could not be had") : laid, "laying out the bins it owns")) return s;
    const size_t bins_y = p.nbins / p.bins_x, fh = (size_t)c->fh, fw = (size_t)c->fw;
    std::vector<size_t> lo((size_t)world), hi((size_t)world);          // (an owner owns whole bin rows)
    for (int r = 0; r < world; ++r) {
        lo[(size_t)r] = std::min(fh, (bins_y * (size_t)r / (size_t)world) << th::kBinShift) * fw;
        hi[(size_t)r] = std::min(fh, (bins_y * ((size_t)r + 1) / (size_t)world) << th::kBinShift) * fw;
    }
    return gather_owned(c, view, both, lo, hi);
}

// ---- th_draw_sharded, in its parts -----------------------------------------------------------------------------------------------
// the fixed buffers of the exchange, once - and the ranks make sure that every one of them has them
static th_status sharded_draw_fixed(th_context *c, bool view)
{
    const int world = c->comm_world, W = c->cfg.width;
    if (c->sharded_draw_ready) return view ? view_storage(c) : TH_OK;       // (a resized target: the same on every rank)
    auto fixed = [&]() -> th_status {
        if (th_status s = c->x_counts.reserve(kXWords, kXWords)) return s;
        if (world > 1) if (th_status s = c->x_halo.reserve((size_t)4 * W, (size_t)4 * W)) return s;
        if (th_status s = line_rows(c)) return s;
        if (world > 1 && c->rows_cross_bands) if (th_status s = c->edge_rows.reserve((size_t)4 * W, (size_t)4 * W)) return s;
        return view ? view_storage(c) : TH_OK;
    };
    if (th_status s = agree_status(c, fixed(), "allocating the exchange's buffers")) return s;
    c->sharded_draw_ready = true;
    return TH_OK;
}

// the tail of both halo exchanges: two rows of cur and prev each way are in x_halo - `lo` from the rank below, `hi` from the rank above
static void halo_received(th_context *c)
{
    const int world = c->comm_world, rank = c->comm_rank, W = c->cfg.width;
    const uint64_t rows_moved = 2ull * ((rank > 0 ? 1u : 0u) + (rank + 1 < world ? 1u : 0u)) * (uint64_t)W * sizeof(float4);
    c->last_draw.sent_bytes += rows_moved; c->last_draw.received_bytes += rows_moved;
    c->halo_lo = rank > 0 ? c->x_halo : nullptr;
    c->halo_hi = rank + 1 < world ? c->x_halo + (size_t)2 * W : nullptr;
}

// a job that draws through the bins keeps its slot order: a band's two edge rows are picked out of the slot order
// (th::LineSources) into texel order, f32, and sent from there.  (the gather's out-of-band word is cleared by the
// draw that follows before anyone reads it - kept as it is here)
static th_status halo_exchange_bins(th_context *c, const th_deposit_uniforms *du)
{
    const int world = c->comm_world, rank = c->comm_rank, W = c->cfg.width;
    th::DepositParams p;
    th_status mine = injected(c, 1);
    if (mine == TH_OK) mine = deposit_prepare_bins(c, du, p);
    if (mine == TH_OK) { th::launch_bins_edge_rows(p, c->edge_rows, c->stream); if (hipGetLastError() != hipSuccess) mine = fail(TH_ERR_HIP, "the edge rows' gather could not be launched"); }
    if (th_status s = agree_status(c, mine, "gathering its edge rows")) return s;
    std::vector<size_t> sc((size_t)world, 0), so((size_t)world, 0), rc((size_t)world, 0), ro((size_t)world, 0);
    // to rank - 1: my first row of cur and of prev (its `hi`); to rank + 1: my last rows (its `lo`); two rows of W texels each
    if (rank > 0) { sc[(size_t)rank - 1] = 2; so[(size_t)rank - 1] = 0; rc[(size_t)rank - 1] = 2; ro[(size_t)rank - 1] = 0; }
    if (rank + 1 < world) { sc[(size_t)rank + 1] = 2; so[(size_t)rank + 1] = 2; rc[(size_t)rank + 1] = 2; ro[(size_t)rank + 1] = 2; }
    if (c->transport->alltoallv(c->comm, c->edge_rows, sc.data(), so.data(), c->x_halo, rc.data(), ro.data(), (size_t)W * sizeof(float4), world, c->stream))
        return fail(TH_ERR_UNSUPPORTED, "%s", th::comm_error());
    halo_received(c);
    return TH_OK;
}

// ... and in texel order the rows are sent from the ring itself (a packed ring: from its f32 views - what the stored texels
// decode to, what the lines are made of)
static th_status halo_exchange_stream(th_context *c)
{
    const int world = c->comm_world, rank = c->comm_rank, W = c->cfg.width;
    th_status mine = c->packed ? injected(c, 1) : TH_OK;
    if (mine == TH_OK) mine = ensure_identity(c);
    const float4 *state[2] = {nullptr, nullptr};
    for (int b = 0; b < 2 && mine == TH_OK; ++b) {
        float4 *v = nullptr;
        mine = unpacked_view(c, c->ring[(size_t)b], b, &v);
        state[b] = v;
    }
    // (an f32 ring: nothing here fails on one rank alone - no agreement, no extra round trip)
    if (c->packed) { if (th_status s = agree_status(c, mine, "decoding its packed edge rows")) return s; }
    else if (mine != TH_OK) return mine;
    std::vector<size_t> sc((size_t)world, 0), so((size_t)world, 0), rc((size_t)world, 0), ro((size_t)world, 0);
    for (int b = 0; b < 2; ++b) {           // ring buffer b: one exchange each (the rows lie in different allocations)
        std::fill(sc.begin(), sc.end(), 0); std::fill(rc.begin(), rc.end(), 0);
        // to rank - 1: my first row (its `hi`); to rank + 1: my last row (its `lo`).  Offsets are in rows of W texels from `state`.
        if (rank > 0) { sc[(size_t)rank - 1] = 1; so[(size_t)rank - 1] = 0; rc[(size_t)rank - 1] = 1; ro[(size_t)rank - 1] = (size_t)b; }
        if (rank + 1 < world) { sc[(size_t)rank + 1] = 1; so[(size_t)rank + 1] = (size_t)c->cfg.height - 1; rc[(size_t)rank + 1] = 1; ro[(size_t)rank + 1] = 2 + (size_t)b; }
        if (c->transport->alltoallv(c->comm, state[b], sc.data(), so.data(), c->x_halo, rc.data(), ro.data(), (size_t)W * sizeof(float4), world, c->stream))
            return fail(TH_ERR_UNSUPPORTED, "%s", th::comm_error());
    }
    halo_received(c);
    return TH_OK;
}

th_status th_draw_sharded(th_context *c, const th_deposit_uniforms *du, const th_render_uniforms *ru, uint64_t *fragments)
{
    if (th_status s = use(c)) return s;
    TH_REQUIRE(du, "null uniforms");
    TH_REQUIRE(c->comm, "th_draw_sharded needs the job's communicator (th_comm_init)");
    TH_REQUIRE(c->comm_world <= 32, "the owners' merge handles up to 32 ranks");
    if (ru) if (th_status s = shared_uniforms(du, ru)) return s;      // (the same on every rank: a host error, not a rank-local one)
    const int world = c->comm_world;
    c->last_draw.sent_bytes = c->last_draw.received_bytes = 0;
    if (th_status s = sharded_draw_fixed(c, ru != nullptr)) return s;
    // the neighbouring bands' edge rows of both state buffers (the fp32 row lookup of the vertex stream can land one row
    // beside a line's own row for some texture heights): my first row to the rank below, my last row to the rank above.
    // Through the bins, where every vertex of every line is the line's own particle, a job needs none of this; where the row
    // lookup drifts (rows_cross_bands: a property of the texture's shape, the same on every rank) it does.
    if (th_status s = line_rows(c)) return s;
    const bool bins = binned_shards(c);
    c->halo_lo = c->halo_hi = nullptr;
    if (world > 1 && bins && c->rows_cross_bands) if (th_status s = halo_exchange_bins(c, du)) return s;
    if (world > 1 && !bins) if (th_status s = halo_exchange_stream(c)) return s;
    c->dep_owners = (uint32_t)world;
    auto pass = [&](const th_deposit_uniforms *d, const th_render_uniforms *r, uint64_t *n) -> th_status {
        if (bins) {
            const th_status s = sharded_pass_bins(c, d, r, n);
            if (s != kRetryInStreamOrder) return s;          // (on every rank together: the stream-ordered pass instead)
        }
        const PassSpec one = r ? builtin_pass(TH_PASS_VIEW, r) : builtin_pass(TH_PASS_FLOW, d);      // (d alone: the flow pass; r alone: the view pass)
        return sharded_pass(c, d && r ? nullptr : &one, d, r, n);
    };
    if (ru && drawn_line_width(c, TH_PASS_FLOW) == drawn_line_width(c, TH_PASS_VIEW)) {
        // both passes draw the same lines: one rasterisation, one exchange of fragments carrying both varyings
        if (th_status s = pass(du, ru, fragments)) return s;
    } else {
        if (th_status s = pass(du, nullptr, fragments)) return s;
        if (ru) if (th_status s = pass(nullptr, ru, nullptr)) return s;
    }
    // (no synchronize: like every other entry point the call enqueues and returns - the all-gathers of the owned ranges are
    // on the context's stream, and so is whatever the host asks for next)
    return TH_OK;
}

// th_draw_sharded with a caller's vertex stage in one pass or in both (th_drawprog.hip: th_draw_program_emit): always pass by
// pass and always stream-ordered - two programs need not agree on where the lines are, so there is no paired rasterisation, and
// the bins of a sharded pass carry the built-in stages alone.  A null program: the built-in stage of that pass.  Only the emit
// of sharded_pass differs; what a program's emit can fail at on one rank alone - loading the program, growing the vertex
// buffer, the launch, a halo row nobody holds - reaches every rank with the counts, as a built-in emit's failure does.
th_status th_draw_program_sharded(th_context *c, th_program *flow_program, const void *flow_uniforms, uint32_t flow_bytes, const th_deposit_uniforms *du,
                                  th_program *view_program, const void *view_uniforms, uint32_t view_bytes, const th_render_uniforms *ru,
                                  uint64_t *fragments, uint64_t *view_fragments)
{
    if (th_status s = use(c)) return s;
    TH_REQUIRE(flow_program || view_program, "th_draw_program_sharded without a program: th_draw_sharded draws with the built-in stages");
    if (flow_program) { if (th_status s = program_run_args(flow_program, kDrawProgram, "th_draw_program_sharded", flow_uniforms, flow_bytes)) return s; }
    else TH_REQUIRE(du, "null uniforms: without a flow program the flow pass is the built-in stage's");
    if (view_program) if (th_status s = program_run_args(view_program, kDrawProgram, "th_draw_program_sharded", view_uniforms, view_bytes)) return s;
    TH_REQUIRE(c->comm, "th_draw_program_sharded needs the job's communicator (th_comm_init)");
    TH_REQUIRE(c->comm_world <= 32, "the owners' merge handles up to 32 ranks");
    if (th_status s = texels_fit_keys(c, "target")) return s;          // (the same on every rank: a host error, not a rank-local one)
    const int world = c->comm_world;
    const bool view = view_program != nullptr || ru != nullptr;
    if (fragments) *fragments = 0;
    if (view_fragments) *view_fragments = 0;
    c->last_draw.sent_bytes = c->last_draw.received_bytes = 0;
    if (th_status s = sharded_draw_fixed(c, view)) return s;
    // the neighbours' edge rows, always: which rows a program's lines read is the stream's business, as for the built-in stages
    c->halo_lo = c->halo_hi = nullptr;
    if (world > 1) if (th_status s = halo_exchange_stream(c)) return s;
    c->dep_owners = (uint32_t)world;
    const PassSpec flow = flow_program ? program_pass(TH_PASS_FLOW, flow_program, flow_uniforms, flow_bytes) : builtin_pass(TH_PASS_FLOW, du);
    if (th_status s = sharded_pass(c, &flow, nullptr, nullptr, fragments)) return s;
    if (!view) return TH_OK;
    const PassSpec seen = view_program ? program_pass(TH_PASS_VIEW, view_program, view_uniforms, view_bytes) : builtin_pass(TH_PASS_VIEW, ru);
    return sharded_pass(c, &seen, nullptr, nullptr, view_fragments);
}

// ---- one process per GPU: the communicator of the job's ranks and the path's collective (th_comm.hip) --------------------
th_status th_comm_unique_id(void *id_out)
{
    TH_REQUIRE(id_out, "null output");
    if (th::comm_unique_id(id_out, TH_COMM_ID_BYTES)) return fail(TH_ERR_UNSUPPORTED, "%s", th::comm_error());
    return TH_OK;
}

#ifdef TH_TESTING
th_status th_comm_loopback_id(void *id_out)
{
    TH_REQUIRE(id_out, "null output");
    if (th::loopback_unique_id(id_out, TH_COMM_ID_BYTES)) return fail(TH_ERR_UNSUPPORTED, "%s", th::comm_error());
    return TH_OK;
}
#endif

th_status th_comm_init(th_context *c, const void *id, int32_t rank, int32_t world)
{
    if (th_status s = use(c, true)) return s;
    TH_REQUIRE(id, "null communicator id");
    TH_REQUIRE(world >= 1 && rank >= 0 && rank < world, "rank %d outside world %d", rank, world);
    TH_REQUIRE(!c->comm, "the context already holds a communicator (th_comm_destroy first)");
    if (th_status s = c->d_status.reserve(2, 2)) return s;
    if (th::comm_init(&c->comm, &c->transport, id, TH_COMM_ID_BYTES, rank, world)) return fail(TH_ERR_UNSUPPORTED, "%s", th::comm_error());
    c->comm_rank = rank; c->comm_world = world;
    c->sharded_draw_ready = false;
    return TH_OK;
}

th_status th_comm_destroy(th_context *c)
{
    if (th_status s = use(c, true)) return s;
    if (!c->comm) return TH_OK;
    TH_HIP(hipStreamSynchronize(c->stream));
    const int bad = c->transport->destroy(c->comm);
    c->comm = nullptr; c->transport = nullptr; c->comm_rank = 0; c->comm_world = 1;
    if (bad) return fail(TH_ERR_UNSUPPORTED, "%s", th::comm_error());
    return TH_OK;
}

th_status th_comm_query(th_context *c, th_comm_info *out)
{
    TH_REQUIRE(c && out, "null argument");
    *out = th_comm_info{};
    out->rank = c->comm_rank; out->world = c->comm_world; out->active = c->comm ? (c->transport == nullptr || strcmp(c->transport->name, "rccl") == 0 ? 1 : 2) : 0;
    int v = 0;
    if (th::comm_available(&v) == 0) out->rccl_version = v;
    return TH_OK;
}

// ---- row-band shards: the whole particle texture on every rank, for the spawners that sample arbitrary particles ----------
static th_status gather_storage(th_context *c, int32_t buffer)
{
    TH_REQUIRE(buffer >= 0 && buffer < (int32_t)c->ring.size(), "bad buffer %d (ring has %zu)", buffer, c->ring.size());
    if (!c->gathered) if (th_status s = c->gathered.alloc((size_t)c->cfg.width * c->cfg.global_height)) return s;
    c->gathered_of = nullptr;
    return TH_OK;
}

th_status th_state_gather_ptr(th_context *c, int32_t buffer, void **dptr)
{
    if (th_status s = use(c, true)) return s;
    TH_REQUIRE(dptr, "null output");
    if (th_status s = gather_storage(c, buffer)) return s;
    if (th_status s = ensure_identity(c)) return s;          // (the association below is with the buffer as the host will see it)
    c->gathered_of = c->ring[(size_t)buffer];
    *dptr = c->gathered;
    return TH_OK;
}

th_status th_state_gather(th_context *c, int32_t buffer)
{
    if (th_status s = use(c, true)) return s;
    TH_REQUIRE(c->comm, "th_state_gather needs the job's communicator (th_comm_init)");
    if (th_status s = gather_storage(c, buffer)) return s;
    if (th_status s = ensure_identity(c)) return s;          // bands travel in texel order
    // the bands of sharding.shard_rows: contiguous, balanced (the first H % world ranks hold one row more)
    const int world = c->comm_world, H = c->cfg.global_height, base = H / world, extra = H % world;
    std::vector<size_t> bytes((size_t)world), offset((size_t)world);
    for (int r = 0; r < world; ++r) {
        const int rows = base + (r < extra ? 1 : 0), row0 = r * base + (r < extra ? r : extra);
        bytes[(size_t)r] = (size_t)rows * c->cfg.width * sizeof(float4);
        offset[(size_t)r] = (size_t)row0 * c->cfg.width * sizeof(float4);
        if (r == c->comm_rank)
            TH_REQUIRE(rows == c->cfg.height && row0 == c->cfg.row0, "this context holds rows %d..%d, rank %d of %d balanced bands holds %d..%d",
                       c->cfg.row0, c->cfg.row0 + c->cfg.height, r, world, row0, row0 + rows);
    }
    float4 *data = nullptr;
    if (th_status s = unpacked_view(c, c->ring[(size_t)buffer], 2, &data)) return s;
    if (c->transport->allgather_bytes(c->comm, data, c->gathered, bytes.data(), offset.data(), c->comm_rank, world, c->stream))
        return fail(TH_ERR_UNSUPPORTED, "%s", th::comm_error());
    c->gathered_of = c->ring[(size_t)buffer];
    return TH_OK;
}

// ---- th_spawn_sample on a row-band shard, the taps' texels fetched from the ranks that own them ------------------------------
// (th_kernels.hip: spawn_shard_*_kernel.)  Per chunk of whole rows: taps -> stable partition by owner -> counts, texel indices
// and texels change hands over the context's transport -> the pass's rounds.  What can fail on one rank alone - its scratch,
// a request outside the band of the rank it went to - is agreed on before the next exchange (agree_status): all leave together.
constexpr size_t kSpawnArrayBudget = (size_t)64 << 20;      // bytes of the largest per-tap array (the fetched texels) of one chunk
constexpr size_t kSpawnTapBytes = 4 * sizeof(uint32_t) + sizeof(float4);

// rows of a band fetched at a time: the same on every rank (made of the texture's width, the sample count and the option alone)
static uint32_t spawn_chunk_rows(const th_context *c, int samples)
{
    const size_t per_row = (size_t)c->cfg.width * (size_t)std::max(samples, 1);
    size_t rows = c->opt.spawn_chunk_rows > 0 ? (size_t)c->opt.spawn_chunk_rows : kSpawnArrayBudget / sizeof(float4) / per_row;
    rows = std::min(rows, (((size_t)1 << 30) / per_row));          // (ordinals and sort sizes are 32-bit)
    return (uint32_t)std::max<size_t>(rows, 1);
}

static void spawn_info_local(th_context *c, int samples)
{
    c->last_spawn = th_spawn_info{};
    c->last_spawn.taps = c->last_spawn.local_taps = (uint64_t)std::max(samples, 0) * c->texels();
    c->last_spawn.chunks = 1;
}

th_status th_spawn_sample_sharded(th_context *c, const th_spawn_sample_uniforms *u, int32_t source, int32_t target)
{
    if (th_status s = use(c)) return s;
    TH_REQUIRE(u, "null uniforms");
    if (source < 0 || !c->comm || c->comm_world <= 1) {
        // the spawn data is replicated (flow, image), or the band is the whole texture: the plain pass
        if (th_status s = th_spawn_sample(c, u, source, target)) return s;
        spawn_info_local(c, u->samples);
        return TH_OK;
    }
    // what follows is the same on every rank (a host error is not agreed on: every rank makes it)
    TH_REQUIRE(u->samples >= 0 && u->samples <= 64, "samples out of range");
    TH_REQUIRE(u->apply >= 0 && u->apply <= 3, "unknown apply mode %d", u->apply);
    TH_REQUIRE(c->ring.size() >= 2, "spawn pass needs at least 2 state buffers (have %zu)", c->ring.size());
    TH_REQUIRE(source < (int32_t)c->ring.size(), "bad spawnData source %d", source);
    TH_REQUIRE(target == TH_TARGET_RING || target == TH_TARGET_TARGETS || (target >= 0 && target < (int32_t)c->ring.size()),
               "bad render target %d (ring has %zu buffers)", target, c->ring.size());
    const int world = c->comm_world, rank = c->comm_rank, W = c->cfg.width, H = c->cfg.global_height, samples = u->samples;
    TH_REQUIRE(world <= 32, "the taps are parted for up to 32 ranks");
    TH_REQUIRE((uint64_t)W * (uint64_t)H < (1ull << 32), "a texel index travels in 32 bits: %dx%d is too large", W, H);
    const int base = H / world, extra = H % world;
    {   // the bands of sharding.shard_rows, as th_state_gather checks them
        const int rows = base + (rank < extra ? 1 : 0), row0 = rank * base + std::min(rank, extra);
        TH_REQUIRE(rows == c->cfg.height && row0 == c->cfg.row0, "this context holds rows %d..%d, rank %d of %d balanced bands holds %d..%d",
                   c->cfg.row0, c->cfg.row0 + c->cfg.height, rank, world, row0, row0 + rows);
    }
    const uint32_t chunk_rows = spawn_chunk_rows(c, samples), longest = (uint32_t)(base + (extra ? 1 : 0));
    const uint32_t chunks = std::max(1u, (longest + chunk_rows - 1u) / chunk_rows);
    const uint32_t my_rows = (uint32_t)c->cfg.height;
    c->last_spawn = th_spawn_info{};
    c->last_spawn.chunks = (int32_t)chunks;

    // ---- this rank's buffers: the pass's views of the ring, the target (a staging band when it is the source's storage),
    // scratch for the longest chunk - rank-local, agreed on
    float4 *out = nullptr, *rt = nullptr, *particles = nullptr, *data = nullptr;
    uint32_t *tap_owner = nullptr, *tap_texel = nullptr, *sorted_owner = nullptr, *sorted_ordinal = nullptr;
    float4 *fetched = nullptr;
    bool staged = false;
    auto prepare = [&]() -> th_status {
        if (th_status s = ensure_identity(c)) return s;          // bands are read, asked for and answered in texel order
        if (th_status s = resolve_target(c, target, true, &out)) return s;
        if (th_status s = render_target(c, out, 0, &rt)) return s;
        // (`source` names the buffer in the ring order the pass sees: after the rotation)
        staged = rt == out && out == c->ring[(size_t)source];
        if (staged) { if (th_status s = staging(c, 0, &rt)) return s; }
        if (th_status s = unpacked_view(c, c->ring[1], 1, &particles)) return s;
        if (th_status s = ring_view(c, source, particles, &data)) return s;
        const size_t taps = (size_t)std::min(chunk_rows, my_rows) * (size_t)W * (size_t)samples;
        if (c->sp_taps.size() < taps * kSpawnTapBytes) {
            TH_HIP(hipStreamSynchronize(c->stream));
            if (th_status s = c->sp_taps.alloc(taps * kSpawnTapBytes)) return s;
        }
        const size_t taps_cap = c->sp_taps.size() / kSpawnTapBytes;
        fetched = reinterpret_cast<float4 *>(c->sp_taps.get());     // (the 16-byte array first)
        tap_owner = reinterpret_cast<uint32_t *>(fetched + taps_cap);
        tap_texel = tap_owner + taps_cap; sorted_owner = tap_texel + taps_cap; sorted_ordinal = sorted_owner + taps_cap;
        if (th_status s = c->sp_words.reserve(66, 66)) return s;
        if (taps) if (th_status s = deposit_temp(c, th::radix_sort_temp_bytes((uint32_t)taps, 0, 5))) return s;
        return TH_OK;
    };
    if (th_status s = agree_status(c, prepare(), "preparing its band", true)) return s;
    unsigned long long *sendc = c->sp_words, *recvc = c->sp_words + 32;
    uint32_t *outside = reinterpret_cast<uint32_t *>(c->sp_words + 64);
    int owner_bits = 1;
    while ((1 << owner_bits) < world) ++owner_bits;

    th::SpawnShardParams p{};
    p.particles = particles; p.out = rt; p.data = data;
    p.width = (uint32_t)W; p.row0 = (uint32_t)c->cfg.row0; p.rows = my_rows; p.global_rows = (uint32_t)H;
    p.wf = (float)W; p.hf = (float)H;
    p.world = (uint32_t)world; p.base = (uint32_t)base; p.extra = (uint32_t)extra;
    p.u = *u;
    p.accepted = c->d_respawned + (target == TH_TARGET_TARGETS ? 1 : 0);
    p.owner = tap_owner; p.texel = tap_texel; p.counts = sendc;
    p.fetched = fetched;

    std::vector<size_t> scount((size_t)world), soff((size_t)world), rcount((size_t)world), roff((size_t)world), one((size_t)world, 1), idx((size_t)world);
    for (int r = 0; r < world; ++r) idx[(size_t)r] = (size_t)r;
    for (uint32_t chunk = 0; chunk < chunks; ++chunk) {
        // (a rank with a shorter band joins the last chunks' exchanges with nothing to ask for)
        const uint32_t row_lo = std::min(my_rows, chunk * chunk_rows), row_hi = std::min(my_rows, row_lo + chunk_rows);
        p.first = row_lo * (uint32_t)W; p.count = (row_hi - row_lo) * (uint32_t)W;
        const uint32_t taps = p.count * (uint32_t)samples;
        // stage 1 - the chunk's taps, parted by owner (stable: every owner's part in ordinal order); the counts change hands
        uint32_t *request = tap_owner, *place = sorted_owner;        // (the sort's key buffers, free once it has run)
        auto stage1 = [&]() -> th_status {
            TH_HIP(hipMemsetAsync(c->sp_words, 0, 66 * sizeof(unsigned long long), c->stream));
            if (!taps) return TH_OK;
            th::launch_spawn_shard_taps(p, c->stream);
            // one pass over the owner bits: the result lands in the second pair of buffers
            (void)th::launch_radix_sort_u32(tap_owner, nullptr, sorted_owner, sorted_ordinal, taps, 0, owner_bits, c->dep_temp, true, c->stream);
            th::launch_spawn_shard_requests(sorted_ordinal, tap_texel, request, place, taps, c->stream);
            TH_HIP(hipGetLastError());
            return TH_OK;
        };
        th_status mine = stage1();
        if (c->transport->alltoallv(c->comm, sendc, one.data(), idx.data(), recvc, one.data(), idx.data(), sizeof(unsigned long long), world, c->stream))
            return fail(TH_ERR_UNSUPPORTED, "%s", th::comm_error());
        std::vector<unsigned long long> words(64, 0ull);
        {
            const std::string why = mine != TH_OK ? last_error() : std::string();
            if (th_status s = read_back(c, words.data(), c->sp_words, words.size() * sizeof(unsigned long long))) return s;
            if (mine != TH_OK) last_error() = why;
        }
        size_t at = 0, arriving = 0, asked = 0;
        for (int r = 0; r < world; ++r) {
            const size_t mine_for_r = mine == TH_OK ? (size_t)words[(size_t)r] : 0, theirs = (size_t)words[32 + (size_t)r];
            soff[(size_t)r] = at; at += mine_for_r;
            scount[(size_t)r] = r == rank ? 0 : mine_for_r;
            rcount[(size_t)r] = r == rank ? 0 : theirs;
            roff[(size_t)r] = arriving; arriving += rcount[(size_t)r];
            asked += scount[(size_t)r];
        }
        // stage 2 - room for what the others ask of this rank; the last thing before the requests travel that can fail here alone
        auto stage2 = [&]() -> th_status {
            if (at != (size_t)taps) return fail(TH_ERR_HIP, "the owners' counts (%zu) do not add up to the chunk's %u taps", at, taps);
            if (arriving >= ((size_t)1 << 31)) return fail(TH_ERR_UNSUPPORTED, "too many requests for one owner");
            if (c->sp_asked.size() < arriving) {          // (the requests last: they are only there when the answers are)
                c->sp_asked.reset();
                const size_t cap = arriving + arriving / 4 + 1024;
                if (th_status s = c->sp_answers.alloc(cap)) return s;
                if (th_status s = c->sp_asked.alloc(cap)) return s;
            }
#ifdef TH_TESTING
            if (c->opt.inject_failure == 5 && asked) {          // the first request that leaves: a texel of THIS rank's band
                c->opt.inject_failure = 0;
                size_t first = 0;
                for (int r = 0; r < world; ++r) if (scount[(size_t)r]) { first = soff[(size_t)r]; break; }
                th::launch_exchange_word(request + first, (uint32_t)c->cfg.row0 * (uint32_t)W, c->stream);
                TH_HIP(hipGetLastError());
            }
#endif
            return TH_OK;
        };
        if (mine == TH_OK) mine = stage2();
        if (th_status s = agree_status(c, mine, "parting its taps and making room for the requests", true)) return s;
        // stage 3 - the requests travel; every owner answers out of its band, and says so when it was asked for something else
        if (c->transport->alltoallv(c->comm, request, scount.data(), soff.data(), c->sp_asked, rcount.data(), roff.data(), sizeof(uint32_t), world, c->stream))
            return fail(TH_ERR_UNSUPPORTED, "%s", th::comm_error());
        auto stage3 = [&]() -> th_status {
            th::launch_spawn_shard_answers(data, (uint32_t)c->cfg.row0 * (uint32_t)W, my_rows * (uint32_t)W, c->sp_asked, c->sp_answers, (uint32_t)arriving, outside, c->stream);
            TH_HIP(hipGetLastError());
            uint32_t flag = 0;
            if (arriving) if (th_status s = read_back(c, &flag, outside, sizeof flag)) return s;
            if (flag) return fail(TH_ERR_INVALID, "sharded spawn: rank %d was asked for a texel outside its band (rows %d..%d): the ranks do not hold the balanced bands of one texture",
                                  rank, c->cfg.row0, c->cfg.row0 + c->cfg.height);
            return TH_OK;
        };
        if (th_status s = agree_status(c, stage3(), "answering the requests for its band", true)) return s;
        // stage 4 - the texels come back to the places their requests left from; the pass's rounds over them
        if (c->transport->alltoallv(c->comm, c->sp_answers, rcount.data(), roff.data(), fetched, scount.data(), soff.data(), sizeof(float4), world, c->stream))
            return fail(TH_ERR_UNSUPPORTED, "%s", th::comm_error());
        p.place = place;
        th::launch_spawn_shard_pick(p, c->stream);
        TH_HIP(hipGetLastError());
        c->last_spawn.taps += taps;
        c->last_spawn.local_taps += taps - asked;
        c->last_spawn.sent_bytes += asked * sizeof(uint32_t) + arriving * sizeof(float4);
        c->last_spawn.received_bytes += arriving * sizeof(uint32_t) + asked * sizeof(float4);
    }
    // (every rank has answered the last chunk's requests by now: the source may be written)
    if (staged) TH_HIP(hipMemcpyAsync(out, rt, c->texels() * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    return staged ? TH_OK : commit_target(c, out, rt);
}

th_status th_spawn_query(th_context *c, th_spawn_info *out)
{
    TH_REQUIRE(c && out, "null argument");
    *out = c->last_spawn;
    return TH_OK;
}

th_status th_stats_allreduce(th_context *c)
{
    if (th_status s = use(c, true)) return s;
    if (!c->comm) return TH_OK;                    // a single-rank job: the local block is the global one
    if (c->transport->allreduce_counters(c->comm, c->d_counters, c->stream)) return fail(TH_ERR_UNSUPPORTED, "%s", th::comm_error());
    return TH_OK;
}

th_status th_stats_global(th_context *c, float speed_limit, th_counters *out)
{
    TH_REQUIRE(out, "null output");
    if (th_status s = th_stats_async(c, speed_limit, nullptr)) return s;
    if (th_status s = th_stats_allreduce(c)) return s;
    return read_back(c, out, c->d_counters, sizeof *out);
}

}  // extern "C"
