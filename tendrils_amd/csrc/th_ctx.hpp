// th_ctx.hpp - what the translation units behind include/tendrils_hip.h share: the context, the error helpers and the
// internal functions one unit offers the others (namespace thi).  Host side only; the kernels' interface is th_kernels.hpp.
//   th_mem.hpp    DevBuf / HostBuf: the owner of every device / pinned buffer here (the ring elements apart)
//   th_api.hip    context life cycle, textures, read-backs, timers, options
//   th_order.hip  tile-sorted slot orders of the ring buffers, captured th_step_n graphs
//   th_step.hip   Particles.step: th_step / th_step_n
//   th_spawn.hip  the spawners, and what a pass over the ring starts from: its buffers (RingPass), its spawnData (spawn_data)
//   th_draw.hip   Tendrils.draw(): flow pass, view pass, trail export (binned and stream-ordered pipeline)
//   th_shard.hip  row-band shards: emit / merge, th_draw_sharded, the job's communicator, gathers, counter all-reduce, the sampled spawn
//   th_program.hip user programs: a caller's HIP pass compiled through hiprtc (th_program_compile / _run), and what the four kinds of
//                  program share: the hiprtc binding, the compile, the log, the per-context modules
//   th_screen.hip  screen programs: a caller's HIP pass over a view image, the colour map or a texture (th_screen_program_compile / th_screen_run)
//   th_drawprog.hip draw programs: a caller's vertex stage in one pass of draw() (th_draw_program_compile / th_draw_program_run)
//   th_stepprog.hip step programs: n steps of a caller's integrator in one launch (th_step_program_compile / th_step_program_run)
//   th_measure.hip measure programs: a caller's reduction over a ring buffer (th_measure_program_compile / th_measure_run / _async / _global)
//   th_density.hip the density map: the particles' count and summed velocity on a grid, into a texture slot or the spawn image (th_density / _async)
//   th_select.hip  select: the particles of a ring buffer that match a fixed predicate, as records in texel order (th_select / _async)
//   th_histogram.hip the histogram: the matching particles counted per bin of one scalar of the state (th_histogram / _async);
//                  th_select_match.hpp is what the two units share - the predicate and the checks of its block
//   th_follow.hip  follow: the states of a chosen set of particles, sample by sample, in a history kept on the device
//                  (th_follow_set / _sample / _read / _query); the slots of the set in a tile-sorted order, found when the order changes
//   th_ring.hpp    what the last five units - the passes that read a ring buffer where it lies - share, on the device and on the host
//   th_blend.hip  the demo's colour-map blend and the caller's textures it reads (th_colormap_blend, th_texture_upload); the TH_VIEW_*
//                 names as images (view_image)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "th_kernels.hpp"
#include "th_math.hpp"
#include "th_program_kinds.hpp"

namespace thi {
struct FlowLineScratch;                   // th_flowline.hip
th_status fail(th_status code, const char *fmt, ...);      // records the message th_last_error() returns; returns `code`
std::string &last_error();
}  // namespace thi

#define TH_HIP(expr)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return thi::fail(TH_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define TH_REQUIRE(cond, ...)                            \
    do {                                                 \
        if (!(cond)) return thi::fail(TH_ERR_INVALID, __VA_ARGS__); \
    } while (0)

#include "th_mem.hpp"                     // thi::DevBuf / thi::HostBuf: every device and pinned buffer below is one of these
using thi::DevBuf;
using thi::HostBuf;

// A set of LOCAL TEXELS on the device: a bit per texel in 64-bit words, and the members before each word - the words' popcounts,
// scanned in place (th_sort.hip: launch_texel_set_rank), with the scan's block sums.  A member's rank is th_ring.hpp's texel_rank.
namespace thi {
struct TexelSetView { const unsigned long long *mask; const uint32_t *counts; };      // ... as a kernel reads it
struct TexelSet {
    DevBuf<unsigned long long> mask;
    DevBuf<uint32_t> counts, sums;
    th_status reserve(uint32_t nwords)   // grow-only
    {
        if (th_status s = mask.reserve(nwords, nwords)) return s;
        if (th_status s = counts.reserve(nwords, nwords)) return s;
        return sums.reserve(th::exclusive_scan_sum_words(nwords), th::exclusive_scan_sum_words(nwords));
    }
    TexelSetView view() const { return TexelSetView{mask.get(), counts.get()}; }
};
}  // namespace thi

// Per-context switches (th_option_set / th_option_get).  A context starts from the environment variables of the same
// names, read when it is created - not once per process - so one process can hold contexts on different paths.
struct th_options {
    int bucket = -1;                     // TH_BUCKET: tile-sorted slot order never (0) / always (1) / when it pays (-1)
    int resort_steps = 64;               // TH_RESORT_STEPS: re-sort period of single-step launches
    int rebucket_steps = 256;            // TH_REBUCKET_STEPS: ... of fused launches
    bool fuse = true;                    // TH_FUSE: temporal fusion in th_step_n
    bool graph = true;                   // TH_GRAPH: captured graphs in th_step_n
    bool force_generic = false;          // TH_FORCE_GENERIC: every step through the reference-order kernel
    int draw = -1;                       // TH_DRAW=stream (0) / bins (1): the default of th_draw_pipeline's AUTO
    bool draw_reuse = true;              // TH_DRAW_REUSE: the stream-ordered view pass reuses the flow pass's geometry
    uint32_t bins_pool = 0;              // TH_BINS_POOL: first size of the binned pipeline's page pool (0: by the target's size)
    int bins_pages = 0;                  // TH_BINS_PAGES: pages a bin's list can grow to at first (0: kBinFirstPages); negative: that many and never more
    int inject_failure = 0;              // (tests) the next th_draw_sharded fails on THIS rank at stage 1 / 2 / 3 (5: the next
                                         // th_spawn_sample_sharded asks for a texel outside its owner's band): the ranks must all leave
    bool skip_unseen = true;             // TH_SKIP_UNSEEN: draw() skips the blocks of slots whose lines the step saw end up outside the view (th_step.hip)
    int spawn_chunk_rows = 0;            // TH_SPAWN_CHUNK_ROWS: rows of a band that th_spawn_sample_sharded fetches at a time (0: by the scratch budget)
    bool async_sort = true;              // TH_ASYNC_SORT: a frame loop's re-sort runs beside its draw() instead of inside two of its steps (th_step.hip)
    bool hash_window = true;             // TH_HASH_WINDOW: fused launches hash over a window of the noise lattice where the host can bound it (th_step.hip: hash_window)
    bool stage_bins = false;             // TH_STAGE_BINS: a pass with a caller's fragment stage takes the pipeline the pass without it would (th_draw.hip: deposit_prepare)
    bool line_bins = false;              // TH_LINE_BINS: ... also when the stage reads th_line: line records per place of the page store (th_fragline.hip); nothing without stage_bins
};

// A compiled program of any kind: the gfx950 code object, until th_program_destroy; the record itself lives as long as
// anything names it - the caller (until th_program_destroy) and every context that loaded it (until th_destroy).
struct th_program {
    thi::ProgramKind kind = thi::kStateProgram;
    std::string name;
    std::vector<char> code;
    std::mutex lock;                     // `code` against a th_program_destroy on another thread
    bool destroyed = false;
    std::atomic<int> refs{1};
    uint32_t sgprs = 0, code_bytes = 0;  // of the kind's kernel, read from the code object
    bool reads_line = false;             // a fragment program whose source names th_line (th_fragment_program_compile): its passes write the
                                         // fragments' line records (th_fragline.hip) and launch the entry points that take them
    bool names_flow = false;             // a fragment program whose source names th_flow (th_fragment_program_compile): as the VIEW pass's stage it
                                         // keeps th_draw_stages_pair to two passes - run in sequence it sees the field the flow pass has blended into
};
// ... and as one context has loaded it (th_program.hip): the context owns the module - unloaded when the context goes - and
// a reference to the program's record, so that th_program_destroy of a program a context has run is safe.
namespace thi {
struct ProgramModule {
    th_program *prog = nullptr;
    hipModule_t module = nullptr;
    hipFunction_t entry[kMaxProgramEntries] = {};      // the kind's entry points, by its enumerators (th_program_kinds.hpp: DrawEntry, FragmentEntry, ...)
    ProgramModule() = default;
    ProgramModule(const ProgramModule &) = delete;             // (the context holds each behind a pointer: nothing moves one)
    ProgramModule &operator=(const ProgramModule &) = delete;
    ~ProgramModule() { reset(); }
    void reset();                        // th_program.hip
};
}  // namespace thi

// A caller's fragment stage as one pass carries it (th_fragprog.hip: th_draw_stages_run / _emit load the module): an argument from
// the pass's entry point down to where its fragments lie (deposit_run, deposit_run_bins, emit_parted), null when the pass has none - beside
// th::DepositParams, which is a kernel's argument and knows nothing of it.  Beside a pass that draws BOTH passes from one
// rasterisation (p.mode == 2: th_draw_stages_pair) the same argument points at TWO of these - [0] the flow pass's stage, [1] the
// view pass's, `module` null where that pass has none -, and fragment_stage_run / fragment_stage_run_bins run each over its half.
namespace thi {
struct FragmentStage {
    ProgramModule *module;
    const void *uniforms; uint32_t uniform_bytes;
    int32_t pass;
};
// the stage reads th_line(f): its pass holds a line record per fragment, and is stream-ordered whatever TH_OPT_STAGE_BINS says
// unless TH_OPT_LINE_BINS is on as well
// (the two stages of a mode 2 pass never do: th_draw_stages_pair runs such a program's pass on its own)
inline bool stage_reads_line(const FragmentStage *stage) { return stage && stage->module && stage->module->prog->reads_line; }
// One pass of draw() as its entry point describes it, for pass_run (a whole texture) and pass_emit (a row band; th_draw.hip); both passes in one (th_draw, th_draw_emit) prepare themselves
struct PassSpec {
    int32_t pass = TH_PASS_FLOW;                                                         // TH_PASS_FLOW / TH_PASS_VIEW
    th_program *vertex = nullptr; const void *uniforms = nullptr; uint32_t uniform_bytes = 0;      // the vertex stage: a draw program and its block, or null:
    const void *builtin = nullptr;                                                       // ... the library's own, with its th_deposit_uniforms (flow) / th_render_uniforms (view)
    const FragmentStage *fragment = nullptr;                                             // the fragment stage, or null
};
inline PassSpec builtin_pass(int32_t pass, const void *uniforms) { PassSpec s; s.pass = pass; s.builtin = uniforms; return s; }
inline PassSpec program_pass(int32_t pass, th_program *prog, const void *u, uint32_t bytes) { PassSpec s; s.pass = pass; s.vertex = prog; s.uniforms = u; s.uniform_bytes = bytes; return s; }
}  // namespace thi

// One captured th_step_n sequence (see th_step_n).
struct GraphEntry {
    int32_t n = 0;
    th::LogicVariant variant{};          // the kernels the sequence launches
    bool generic = false;
    std::vector<float4 *> ring;          // ring order at capture time
    th::LogicParams key{};               // launch parameters (the fields same_key() compares)
    hipGraphExec_t exec = nullptr;
    DevBuf<float> times_dev;
    HostBuf<float> times_host;
    hipEvent_t copied = nullptr;         // times_host -> times_dev copy of the last replay
};

struct th_context {
    th_config cfg{};
    th_options opt{};
    hipStream_t stream = nullptr;
    std::vector<float4 *> ring;          // ring[0] = buffers[0] (most recent); TH_STATE_F16: packed, 8 B per texel
    bool packed = false;                 // cfg.state_format == TH_STATE_F16
    DevBuf<float4> tmp[3];               // f32 staging for the non-hot operations on a packed ring
    DevBuf<float4> flow;
    DevBuf<float2> flow_dec;             // per-step decoded plane (launch_flow_decode)
    DevBuf<float> flow3;                 // the flow texels' x, y, z alone (fused passes: th_step_n packs them once per call)
    int32_t fw = 0, fh = 0;
    DevBuf<float4> targets;
    bool targets_checked = true, targets_nonfinite = false;   // fresh texture = zeros
    DevBuf<float4> lut_block;            // [hash tables | gradient table] ...
    float4 *lut = nullptr;               // ... the gradient table inside it
    DevBuf<float4> win_block;            // [winA | winB | winG]: the same tables extended periodically (th_logic.hpp "over a window")
    long long dense_sorts = 0;           // plain re-sorts whose passes counted densely in LDS (TH_OPT_DENSE_SORTS)
    long long hash_window_launches = 0;  // fused launches that ran over the window tables (TH_OPT_HASH_WINDOW_LAUNCHES)
    DevBuf<uchar4> frames[2];
    int32_t frw = 0, frh = 0;
    DevBuf<unsigned int> d_flag;
    DevBuf<th::StatsPartial> partials;
    // the statistics a fused th_step_n launch took of the state it wrote (LogicParams::stats_part): valid while ring[0] is
    // that buffer and nothing has written it (use() without keeps_lines drops them)
    DevBuf<th::StatsPartial> fused_parts;
    struct { bool valid = false; const float4 *buf = nullptr; float limit = 0.0f; uint32_t nparts = 0; } fused_stats;
    DevBuf<th_counters> d_counters;
    // th_draw_sharded: the neighbours' edge rows, the owners' counts, what this rank received
    DevBuf<float4> x_halo;               // [lo: cur row, prev row | hi: cur row, prev row], `width` texels each
    DevBuf<unsigned long long> x_counts;   // device: bounds (33) | send counts (32) | recv counts (32)
    DevBuf<unsigned long long> x_keys;   // (x_keys.size() is the capacity of both: exchange_room)
    DevBuf<float4> x_colors;
    DevBuf<float4> gathered;             // row-band shard: a copy of the WHOLE particle texture (th_state_gather / _ptr) ...
    const void *gathered_of = nullptr;   // ... of this ring buffer, for the spawners that sample arbitrary particles
    // th_spawn_sample_sharded (th_shard.hip): per tap of a chunk four u32 arrays and the fetched texels; what the other ranks
    // ask this one for, and its answers; the counts' words (send 32 | receive 32 | the out-of-band flag)
    DevBuf<char> sp_taps;                // (kSpawnTapBytes per tap)
    DevBuf<uint32_t> sp_asked;           // (sp_asked.size() is the capacity of both)
    DevBuf<float4> sp_answers;
    DevBuf<unsigned long long> sp_words;
    th_spawn_info last_spawn{};          // th_spawn_query
    void *comm = nullptr;                // communicator of the job's ranks (th_comm_init), one rank per context ...
    const th::Transport *transport = nullptr;   // ... and how its ranks exchange bytes (RCCL; in-process for tests)
    DevBuf<uint32_t> d_status;           // the word the ranks agree on (agree_status)
    DevBuf<uint32_t> own_mem;            // th_draw_sharded through the bins: counts, offsets, tables (th_bins.hip: OwnerParams)
    bool sharded_draw_ready = false;     // th_draw_sharded has allocated its fixed buffers (and the ranks agreed that all did)
    int32_t comm_rank = 0, comm_world = 1;
    // flow deposit scratch (grow-only): per-flow-texel counters and the fragment lists
    DevBuf<uint32_t> dep_count, dep_offset, dep_blocks, dep_total;   // per line; scan scratch
    DevBuf<uint4> dep_record;            // per line: the texels of a short line
    DevBuf<uint32_t> dep_lists;          // slow / long line lists (counters first)
    uint32_t dep_owners = 1;             // th_deposit_set_owners: ranks owning flow texels in the sharded deposit
    bool dep_pairs = false;              // the colour buffers hold two varyings per fragment (th_draw)
    // the geometry of the last draw pass (fragment counts, offsets, records, the sorted fragment order): the flow pass
    // and the view pass of one draw() rasterise the same lines at the same resolution
    float line_width[2] = {1.0f, 1.0f}, line_range[2] = {1.0f, 1.0f};     // th_line_width (per pass: TH_PASS_FLOW, TH_PASS_VIEW) / th_line_width_range
    struct { bool valid = false, binned = false; float view_x = 0, view_y = 0, line_half = 0; uint32_t total = 0, nlarge = 0, nblocks = 0; bool sorted_in_a = false; } drawn;
    uint32_t dep_list_cap = 0;
    // binned pipeline (th_bins.hip): the bins' cursors | the large bins | first block of each (+ 1) | first regrouped key of each (+ 1)
    DevBuf<uint32_t> bin_mem;
    uint32_t bin_capacity = 0;
    DevBuf<uint32_t> chunk_table;        // per list x bin_max_pages: the pages a list has grown by
    // the blocks of 256 slots with a line that can draw, for the slot order ring[0] is held in (th_bins.hip: bins_block_list_kernel)
    DevBuf<uint32_t> draw_blocks;
    uint32_t draw_nblocks = 0;
    DevBuf<uint8_t> draw_block_flags;
    int draw_blocks_order = -2;
    unsigned long long draw_blocks_stamp = 0;
    // ... and the same list for TEXEL order, an entry of its own: a draw program's binned pass walks its vertex records in texel
    // order whatever order the ring is held in, and a frame that mixes it with a built-in pass over sorted slots would otherwise
    // rebuild a list (a read-back each) twice per frame.  A property of the texture's shape alone: listed once per context.
    DevBuf<uint32_t> texel_blocks;
    uint32_t texel_nblocks = 0;
    bool texel_blocks_listed = false;
    uint32_t bin_max_pages = 0;          // (widened when a bin outgrows its lists: bins_table_widen)
    bool bins_dirty = false;             // an emitting pass filled the store and no blend has emptied it since (a sharded draw that ended
                                         // between the two): the next emitting pass wipes it first
    DevBuf<unsigned long long> bins_keys;      // the page store: (bins x kBinReplicas + bins_pool) pages of kBinPage places - keys (~0 = empty) ...
    DevBuf<float4> bins_colors;          // ... and varyings (two per place once a th_draw has run)
    // TH_OPT_LINE_BINS, reserved by the first binned pass whose stage reads th_line (th_draw.hip: bins_line_store): the lines'
    // snapped endpoints by stream index (W x H x 16 bytes), and a line record per place of the store (16 bytes a place: follows the store)
    DevBuf<int4> bins_line_ends;
    DevBuf<th::FragmentLine> bins_lines;
    size_t bins_lines_places = 0;
    uint32_t bins_pool = 0, bins_store_bins = 0;
    bool bins_pairs = false;
    DevBuf<uint32_t> crowd_mem;          // per large bin: fragments per texel, first fragment of every texel, fill cursors, long runs
    uint32_t crowd_capacity = 0;         // (in bins: where the arrays inside crowd_mem begin)
    DevBuf<unsigned long long> crowd_keys;     // the large bins' fragments regrouped by texel
    DevBuf<uint32_t> crowd_sorted;             // ... their places, run by run in blend order
    DevBuf<unsigned long long> crowd_parted;     // ... the giants' keys parted by stream index, and their windows (th_bins.hip: giant_*_kernel)
    DevBuf<uint32_t> crowd_windows;
    size_t crowd_keys_cap = 0;
    hipStream_t side = nullptr;                // the long runs of a crowded target are blended beside everything else
    hipEvent_t forked = nullptr, joined = nullptr;
    hipStream_t side2 = nullptr;               // ... and the crowded bins' short runs beside both
    hipEvent_t joined2 = nullptr, regrouped = nullptr;
    HostBuf<uint32_t> bins_totals_host;        // (coherent, mapped; kTotWords + 1 words) the binned pass's totals, written by the plan's last kernel, and the sequence number behind them
    uint32_t *bins_totals_dev = nullptr;       // ... as the device addresses it
    uint32_t totals_seq = 0;
    bool mrg_pairs = false, x_pairs = false;   // the merge / exchange colour buffers hold two varyings per fragment (th_draw_emit / _merge)
    HostBuf<char> pinned;                      // (kPinnedBytes) small read-backs: a pageable hipMemcpyAsync costs ~0.15 ms per call
    int lines_local = -1;                // every vertex of every line reads the line's own particle (line_rows)
    DevBuf<uint32_t> d_row_draws;        // bit per global row: the row's lines can draw (line_rows)
    // ... and when not (lines_local == 0): the rows / columns whose texels some OTHER line's vertex reads, and - per slot order -
    // where those texels lie (th::LineSources; th_bins.hip: bins_block_flags_kernel)
    DevBuf<uint16_t> src_row_index, src_col_index;
    uint32_t src_nrows = 0, src_ncols = 0;
    bool rows_cross_bands = false;       // some line of this band looks a row of a neighbouring band up (halo rows needed)
    DevBuf<uint32_t> src_slots;          // (allocated with draw_blocks; valid for draw_blocks_order / _stamp)
    DevBuf<float4> edge_rows;            // th_draw_sharded through the bins: this band's edge rows gathered into texel order (4 x W)
    int draw_pipeline = TH_DRAW_AUTO;    // th_draw_pipeline
    th_draw_info last_draw{};            // th_draw_query
    long long draws = 0;                          // (`draws` counts frames: the passes drawn at one total_steps share a count ...
    long long draw_frame_step = -1;               //  ... and a pipeline: th_draw.hip, draw_uses_bins)
    int frame_bins = -1;
    long long last_binned_draw = -(1ll << 40);   // total_steps at the last draw over slot order
    DevBuf<uint32_t> dep_u32[4];                                     // per fragment: keys, slots, and both sorted
    DevBuf<unsigned long long> dep_u64[2];                           // sharded form: (texel, stream index) keys, sorted
    DevBuf<float4> dep_colors_sorted;
    bool dep_wide = false;
    const float4 *halo_lo = nullptr, *halo_hi = nullptr;             // caller-owned neighbour rows (th_deposit_set_halo)
    DevBuf<unsigned long long> mrg_keys, mrg_keys2;                  // th_deposit_merge scratch (sort ping-pong)
    DevBuf<uint32_t> mrg_vals[2];
    size_t mrg_capacity = 0;
    DevBuf<float4> mrg_colors;           // the received varyings gathered into texel order
    DevBuf<float4> dep_colors;
    DevBuf<th::FragmentLine> dep_fraglines;                          // per fragment: its line's record - only once a pass's fragment stage has read th_line (deposit_reserve)
    DevBuf<char> dep_temp;
    size_t dep_lines = 0, dep_capacity = 0;   // (set once all of their buffers are there: prepare_pass, deposit_reserve)
    uchar4 *view = nullptr;              // the BOUND view image (RGBA8, flow shape): what the view pass, fills, clears and read-backs touch
    int32_t view_w = 0, view_h = 0;
    DevBuf<uchar4> view_screen;          // the drawing buffer (bound unless th_view_bind chose a buffer), lazily allocated
    std::vector<uchar4 *> view_ring;     // Tendrils.buffers (src/index.js:172-184): off-screen view images, in ring order
    int32_t view_buffers = 0;            // how many the host asked for (th_view_buffers)
    int32_t view_bound = -1;             // ring position of the bound image when it was bound; -1: the screen (the pointer `view` is what counts)
    DevBuf<float4> colormap;             // tendrils.colorMap (nullptr = the 1x1 zero texture)
    int32_t cmap_w = 0, cmap_h = 0;
    DevBuf<float4> image;                // PixelSpawner's own buffer (TH_SOURCE_IMAGE)
    int32_t iw = 0, ih = 0;
    // the caller's textures (th_texture_upload): what the colour-map blend sums beside the frames and the spawn image (th_blend.hip)
    struct Texture { DevBuf<char> texels; int32_t w = 0, h = 0, format = -1; };      // TH_TEX_*: 16 / 4 / 4 bytes a texel
    Texture textures[TH_MAX_TEXTURES];
    DevBuf<unsigned long long> d_respawned;      // [0]: particles replaced by respawn passes, [1]: scratch (passes into `targets`)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool kernel_timing = false;          // th_kernel_timing: event pair around every logic launch (and a draw program's vertex kernel)
    std::vector<hipEvent_t> kt_events;   // pairs (start, stop); kt_used of them recorded
    size_t kt_used = 0;
    std::vector<GraphEntry> graphs;      // th_step_n cache

    // Tile-sorted slot orders (th_kernels.hip "Tile-sorted slot order"); lazily allocated.  Every ring buffer is in
    // texel order or in one of `orders` (a step that re-sorts writes its output in a new order while its input keeps
    // the old one, so two orders can be alive at a time).
    struct SlotOrder {
        DevBuf<uint32_t> perm;               // slot -> particle id
        DevBuf<th::TileChunk> chunks;        // chunk table
        DevBuf<th::ChunkRecord> records;     // per chunk: tiles of the next positions (written by a COUNT pass)
        DevBuf<uint32_t> nchunks;
        th::TileGeom geom{};                 // key function the order was sorted with
        int32_t fw = 0, fh = 0;
        int refs = 0;                        // ring buffers stored in this order
        unsigned long long stamp = 0;        // c->sorts when the order was laid out (what is cached per order - the draw's block list - knows it by this)
    };
    std::vector<SlotOrder> orders;
    std::vector<std::pair<float4 *, int>> buf_order;   // ring buffers held in a sorted order (absent = texel order)
    float4 *spare = nullptr;             // spare state buffer (ensure_identity moves through it: it trades places with ring elements - raw, like them)
    DevBuf<uint32_t> tile_mem;           // hist | cursor (kSortReplicas x kMaxTileBins words each) | misses (8 words) | totals | starts (kMaxTileBins each)
    DevBuf<th::ChunkRecord> block_records;      // per 4096-slot block: tile_hist's table for tile_scatter
    uint32_t max_chunks = 0;
    int steps_since_sort = 0;
    unsigned long long sorts = 0;
    long long total_steps = 0, hold_texel_order_until = 0;   // texel-order consumers (draw) keep the layout off for a period
    bool step_keyed = false;             // th_step_program_view_size: a step program's calls sort the slots themselves, under the
    float step_view[2] = {1.0f, 1.0f};   // ... key of this view size
    HostBuf<uint32_t> miss_host;         // window misses since the last sort, as of some recent launch
    // A re-sort under way beside a draw() (th_step.hip "the re-sort of a frame loop"): the step's output `src` (held in order
    // `src_order`) is being copied into `dst` in the new order `order` on the side stream; the next step takes the copy for
    // its input when nothing has touched `src` since (state_written / state_moved), anything else drops it.
    struct {
        bool pending = false, valid = false;
        const float4 *src = nullptr;
        int src_order = -1, order = -1;
        float4 *dst = nullptr;               // (allocated once; trades places with ring[1]: raw, like the ring elements)
        hipEvent_t ready = nullptr, done = nullptr;
        long long at_step = -1;              // total_steps when it was started
    } asort;
    // what a single step saw of its lines (LogicParams::seen): valid for a draw() that reads exactly these two buffers in this
    // order through this view
    struct {
        DevBuf<uint8_t> bytes;               // texels / 64 of them (a multiple of 4)
        const float4 *cur = nullptr, *prev = nullptr;
        int order = -1;
        unsigned long long stamp = 0;
        float view_x = 0, view_y = 0;
        int32_t fw = 0, fh = 0;
    } seen;
    // a COUNT pass has histogrammed the tiles of the state it wrote: valid for a SCATTER pass that reads exactly that
    struct { const float4 *buf = nullptr; int order = -1; th::TileGeom geom{}; long long at_step = -1; } counted;

    thi::FlowLineScratch *flow_lines = nullptr;   // th_flow_lines: staging and scratch (grow-only)

    std::vector<std::unique_ptr<thi::ProgramModule>> programs;     // th_program_run / th_screen_run / th_draw_program_run: the programs this context has loaded
    DevBuf<unsigned> prog_flag;                   // ... and the word a pass on a row band raises (th_particles outside the band)

    // th_measure_run / _async / _global (th_measure.hip), reserved by the first measure of the context: a partial per workgroup of
    // the caller's kernel (2048), and the result blocks - this context's | the ranks', gathered | the job's
    DevBuf<th_measure_result> measure_parts, measure_blocks;

    // th_density / _async (th_density.hip), reserved by the first density of the context: the cells' accumulators - 20 bytes a
    // cell, in 16-byte words, grow-only - and the info block the call leaves (a th_density_info)
    DevBuf<uint4> density_acc;
    DevBuf<unsigned long long> density_info;

    // th_select / _async (th_select.hip), reserved by the first select of the context: the matching texels, the info block the call leaves (a
    // th_select_info), and the records (grow-only: the largest capacity asked)
    thi::TexelSet select_set;
    DevBuf<unsigned long long> select_info;
    DevBuf<th_selected> select_records;

    // th_histogram / _async (th_histogram.hip), reserved by the first histogram of the context: TH_HIST_MAX_BINS counts and the
    // info block the call leaves (a th_histogram_info)
    DevBuf<uint32_t> hist_counts;
    DevBuf<unsigned long long> hist_info;

    // th_follow_set / _sample / _read / _query (th_follow.hip), reserved by the first th_follow_set of the context: the set as a
    // TexelSet of its own - select's device addresses stay valid until the next select
    // - and as its local texels in set order; the slot of every member in the order `follow.order` / `.stamp`
    // names (-1: texel order, where the texel is the slot; -2: nothing yet); the history, float4[depth][n], row k % depth
    // holding sample k; the callers' times of the samples, by the same row
    thi::TexelSet follow_texels;
    DevBuf<uint32_t> follow_set, follow_slots;
    DevBuf<float4> follow_history;
    struct {
        uint64_t n = 0, depth = 0, samples = 0, locates = 0;
        int order = -2;
        unsigned long long stamp = 0;
        std::vector<double> times;
    } follow;

    // th_draw_program_run: what the caller's vertex stage leaves for the pass - two float4 per stream vertex, 64 B per particle
    // (grows and stays, like the flow lines' scratch)
    DevBuf<float4> draw_vertices;

    size_t texels() const { return (size_t)cfg.width * cfg.height; }
    size_t state_bytes() const { return texels() * (packed ? sizeof(uint2) : sizeof(float4)); }
};

namespace thi {

// ---- th_api.hip ------------------------------------------------------------------------------------------------------
inline bool is_pow2(uint32_t v) { return v && !(v & (v - 1)); }
inline uint32_t ilog2(uint32_t v) { uint32_t r = 0; while (v >>= 1) ++r; return r; }
th_status use(th_context *c, bool keeps_lines = false);
void flow_lines_free(th_context *c);      // th_flowline.hip
th_status alloc_state(th_context *c, float4 **out);
th_status resolve_target(th_context *c, int32_t target, bool rotate_ok, float4 **out);
th_status rect_ok(th_context *c, int32_t x0, int32_t y0, int32_t w, int32_t h);
th_status staging(th_context *c, int k, float4 **out);
th_status unpacked_view(th_context *c, float4 *buf, int k, float4 **out);
th_status render_target(th_context *c, float4 *buf, int k, float4 **out);
th_status commit_target(th_context *c, float4 *buf, float4 *rendered);
constexpr size_t kPinnedBytes = 1024;
th_status read_back(th_context *c, void *host, const void *dev, size_t bytes);
// a whole device image from / to the caller's memory, and the wait for it: `host` is the caller's again when the call returns
th_status image_copy(th_context *c, void *dst, const void *src, size_t bytes, hipMemcpyKind kind);
inline th_status image_upload(th_context *c, void *dev, const void *host, size_t bytes) { return image_copy(c, dev, host, bytes, hipMemcpyHostToDevice); }
inline th_status image_download(th_context *c, void *host, const void *dev, size_t bytes) { return image_copy(c, host, dev, bytes, hipMemcpyDeviceToHost); }
// A device image takes another shape: what the stream still does with the old texels ends first, the stored shape is 0 x 0 while
// there is no storage, then `per_texel` elements of `buf` a texel (uninitialised).  The shape's limits are the entry point's own.
template <class T> th_status image_reshape(th_context *c, DevBuf<T> &buf, int32_t &w, int32_t &h, int32_t new_w, int32_t new_h, size_t per_texel = 1)
{
    TH_HIP(hipStreamSynchronize(c->stream));
    w = h = 0;
    if (th_status s = buf.alloc((size_t)new_w * new_h * per_texel)) return s;
    w = new_w; h = new_h;
    return TH_OK;
}
// the gathered whole-texture copy (th_state_gather / _ptr) is a copy of one ring buffer's CONTENT: writing that buffer ends
// its validity, moving the content to another allocation (slot-order moves through `spare`) takes the association along
inline void state_written(th_context *c, const float4 *buf)
{
    if (c->gathered_of == (const void *)buf) c->gathered_of = nullptr;
    if (c->asort.src == buf) c->asort.valid = false;          // (a re-sort of that content under way: its copy is stale)
    if (c->seen.cur == buf || c->seen.prev == buf) c->seen.cur = c->seen.prev = nullptr;
}
inline void state_moved(th_context *c, const float4 *from, const float4 *to)
{
    if (c->gathered_of == (const void *)from) c->gathered_of = to;
    if (c->asort.src == from) c->asort.valid = false;
    if (c->seen.cur == from || c->seen.prev == from) c->seen.cur = c->seen.prev = nullptr;
}

// Particles.step's rotation (utils.step: pop -> unshift): the last buffer becomes buffers[0]
inline float4 *ring_rotate(th_context *c) { std::rotate(c->ring.begin(), c->ring.end() - 1, c->ring.end()); return c->ring[0]; }

// ---- th_spawn.hip ----------------------------------------------------------------------------------------------------
// one of the ring's buffers as a pass samples it: f32 texels - `particles` itself when k is 1 (the view of ring[1] the pass
// already holds), else the buffer's f32 view in staging slot 2
th_status ring_view(th_context *c, int32_t k, float4 *particles, float4 **out);
// A pass's spawnData by name: TH_SOURCE_FLOW, TH_SOURCE_IMAGE, ring buffer k in the ring order the pass sees (after the
// rotation) - on a row band the gathered copy of the whole texture, if it is of that buffer - or, where the pass can do
// without (none_ok), TH_SOURCE_NONE: no texels, 1 x 1
th_status spawn_data(th_context *c, int32_t source, float4 *particles, bool none_ok, const float4 **data, int32_t *dw, int32_t *dh);
// What a pass over the ring (in texel order: ensure_identity; at least 2 buffers: the caller's check) works on: the target `out` -
// the ring rotated for TH_TARGET_RING -, where the pass writes it (`rt`: staging when packed) and the f32 view of `particles` =
// ring[1], which the pass reads like every Particles.step (src/particles.js:139); commit() packs `rt` into `out`
struct RingPass {
    float4 *out = nullptr, *rt = nullptr, *particles = nullptr;
    th_status begin(th_context *c, int32_t target);
    th_status commit(th_context *c) { return commit_target(c, out, rt); }
};

// ---- th_step.hip -----------------------------------------------------------------------------------------------------
// th_kernel_timing: begin() records the first event of the next pair in front of a launch if timing is on (and `on`: captured
// launches are never bracketed), end() the second behind it
struct LaunchTimer {
    hipEvent_t k1 = nullptr;
    th_status begin(th_context *c, bool on = true);
    th_status end(th_context *c);
};
// One fused launch of m steps on a two-buffer ring: `in` = buffers[0]; state m goes to `out`, state m - 1 to `out_prev` (one is
// `in`, one `other`) - buffers[0] and [1] once fused_routed() has flipped the ring (m odd) and advanced the step counters
struct FusedRoute { float4 *in, *out, *out_prev, *other; };
FusedRoute fused_route(th_context *c, int32_t m);
void fused_routed(th_context *c, int32_t m);

// ---- th_program.hip --------------------------------------------------------------------------------------------------
constexpr uint32_t kUniformBytes = 1024;        // a program's uniform block (th_program_uniform_block in the preludes)
inline const char *program_kind_name(ProgramKind kind) { return kProgramKindTable[kind].what; }
// `prelude` + `#line 1 "<name>"` + `source` through hiprtc into a program of `kind`; th_program_log() holds the compiler's output
th_status program_compile(ProgramKind kind, const std::string &prelude, const char *source, const char *name, th_program **out);
// the checks every run of a program starts with: the handle, its kind (`entry`: the entry point asked), the uniform block
th_status program_run_args(const th_program *prog, ProgramKind kind, const char *entry, const void *uniforms, uint32_t uniform_bytes);
// the context's module of `prog`, loaded on first use
th_status program_loaded(th_context *c, th_program *prog, ProgramModule **out);
// the launch record of a program's kernel: the kind's Args (th_*_args in its prelude), then the uniform block
template <class Args> struct ProgramKernArgs {
    Args a;
    alignas(16) unsigned char u[kUniformBytes];
    void set_uniforms(const void *uniforms, uint32_t bytes) { if (bytes) memcpy(u, uniforms, bytes); }
};
// `fn` over `lanes` lanes (not 0) on the grid of the streaming passes (th::grid_for(lanes, 8)) with the filled record as its
// argument segment: the runtime copies it when it enqueues the launch - no copy of the library's own, nothing to wait for
th_status program_launch(th_context *c, hipFunction_t fn, size_t lanes, void *record, size_t bytes);
template <class Args> th_status program_launch(th_context *c, hipFunction_t fn, size_t lanes, ProgramKernArgs<Args> &k) { return program_launch(c, fn, lanes, &k, sizeof k); }
// ... on a grid of the caller's (256-lane workgroups): a step program over tile-sorted slots takes the built-in fused launch's
th_status program_launch_grid(th_context *c, hipFunction_t fn, int grid, void *record, size_t bytes, int grid_y = 1);
// ---- th_drawprog.hip -------------------------------------------------------------------------------------------------
// s.vertex over the lines of the (prepared) pass `p`, into the vertex buffer its raster stage draws from: a local pass's over the order its pipeline walks (bins: the slots), a band's by local row
th_status vertex_stage_run(th_context *c, const PassSpec &s, th::DepositParams &p, bool bins);
th_status vertex_stage_band(th_context *c, const PassSpec &s, th::DepositParams &p);
// ---- th_fragprog.hip -------------------------------------------------------------------------------------------------
// `stage` over the `total` fragments (not 0) the scatter of the (prepared) pass `p` has just written: p.keys64 / p.keys and
// p.colors, fragment i in place i of both - before anything sorts or parts them.  A stage that reads th_line: the line kernel
// (th_fragline.hip) fills c->dep_fraglines first - reserved by the caller, deposit_reserve(..., lines) - and the stage's line entry points run
th_status fragment_stage_run(th_context *c, const FragmentStage &stage, const th::DepositParams &p, uint32_t total);
// ... and over the fragments an emitting attempt of the binned pass `p` (not mode 2) has just left in the page store: p.frag_keys /
// p.colors at every place the bins' lists handed out - before anything blends, whether or not the host accepts the attempt
// (crowded: the last draw put most of its fragments into crowded bins - a bin's places are dealt to more workgroups; program:
// the pass's vertex stage was a caller's).  A stage that reads th_line: the two line kernels of th_fragline.hip fill
// c->bins_line_ends and c->bins_lines first - reserved by the caller, bins_pass_emit - and the stage's kFragmentLineBins entry point runs.
// p.mode == 2: the pair of both passes' stages, as above, over the two varyings a place of the store then holds
th_status fragment_stage_run_bins(th_context *c, const FragmentStage &stage, const th::DepositParams &p, bool crowded, bool program);
// ---- th_blend.hip ----------------------------------------------------------------------------------------------------
th_status colormap_storage(th_context *c);
// an image a pass taps, as the TH_VIEW_* names resolve: texels in a TH_TEX_* format
struct Image { const void *texels; int32_t w, h, format; };
constexpr uint32_t view_bit(int32_t source) { return 1u << source; }
// (source, index) of the sources in `accepted` (view_bit of each) as an image - the view images and the colour map get their
// storage on the way (view_storage, colormap_storage); what is wrong is said of "<noun> <ordinal>" ("<noun>": ordinal < 0)
th_status view_image(th_context *c, int32_t source, int32_t index, uint32_t accepted, const char *noun, int32_t ordinal, Image *out);
// an RGBA8 image is tapped through a 16-bit fixed-point coordinate (nearest_texel_fx16), which holds 65536 texels a side in 32 bits
constexpr int32_t kRgba8MaxSide = 65536;
inline bool tap_size_ok(const Image &i) { return i.format != TH_TEX_RGBA8 || (i.w <= kRgba8MaxSide && i.h <= kRgba8MaxSide); }

// ---- th_order.hip ----------------------------------------------------------------------------------------------------
void destroy_graph(GraphEntry &g);
void clear_graphs(th_context *c);
constexpr int kTileShift = 5;            // 32 x 32 texel tiles (th_kernels.hip kTile)
constexpr size_t kTileWords = 2 * (size_t)th::kSortReplicas * th::kMaxTileBins;   // histogram + cursors, all copies
bool sorting_possible(const th_context *c);
th_status line_rows(th_context *c);
th::TileGeom tile_geom(const th_context *c, const float viewSize[2]);       // the sort key: the flow tile of pos * viewSize
inline th::TileGeom tile_geom(const th_context *c, const th_logic_uniforms &u) { return tile_geom(c, u.viewSize); }
bool same_geom(const th::TileGeom &a, const th::TileGeom &b);
int order_of(const th_context *c, const float4 *buf);
void set_order(th_context *c, float4 *buf, int order);
bool any_sorted(const th_context *c);
bool order_stale(const th_context *c, int order, const th::TileGeom &g);      // `order` no longer describes the field under `g` (-1: never stale)
void ring_trade(th_context *c, float4 *&slot, float4 *&with, int order);
th_status sort_storage(th_context *c);
th_status asort_drop(th_context *c);
th_status asort_take(th_context *c);
th_status asort_start(th_context *c, const th::TileGeom &g, float4 *src, int src_order);
th_status ensure_identity(th_context *c, bool *launched = nullptr);
th_status begin_sort(th_context *c, const th::TileGeom &g, const float4 *state, const uint32_t *perm_in, int *order,
                     th::TileSortParams *params, bool have_hist = false);
th_status align_slot_orders(th_context *c);
// Slot layout of fused passes (th_step_n, th_step_program_run): see th_order.hip
th_status fused_slots(th_context *c, bool may_sort, const th::TileGeom &g);

// ---- th_draw.hip -----------------------------------------------------------------------------------------------------
int deposit_texel_bits(const th_context *c);
float drawn_line_width(const th_context *c, int pass);
// program: the pass of a caller's draw program (th_drawprog.hip) - its binned form walks the vertex records in texel order over
// a ring left in whatever order it is held in (no perm, no block_seen, no source table, the texel-order block list); stage: the
// pass's fragment stage, or null - with one the pass is stream-ordered, and no frame of the policy's count, unless
// TH_OPT_STAGE_BINS is on and the stage does not read th_line (or TH_OPT_LINE_BINS is on too): then it takes the pipeline the
// pass without the stage would
th_status deposit_prepare(th_context *c, const th_deposit_uniforms *u, th::DepositParams &p, bool want_bins = false, bool *bins = nullptr, bool program = false, const FragmentStage *stage = nullptr);
th_status deposit_scan_total(th_context *c, const th::DepositParams &p, uint32_t *total);
th_status deposit_reserve(th_context *c, uint32_t total, bool wide, bool pairs = false, bool lines = false);      // lines: and a th::FragmentLine per fragment
th_status deposit_temp(th_context *c, size_t need);
// the stream-ordered pipeline over the (prepared) pass `p`: count, scan, emit, `stage` (or null) over the fragments, sort by texel, blend
th_status deposit_run(th_context *c, th::DepositParams &p, const FragmentStage *stage, uint64_t *fragments);
// ... and the binned one (program: p.vertices holds a draw program's records; `stage`, or null, over the page store behind every
// emitting attempt, before anything blends).  kRetryInStreamOrder: see below
th_status deposit_run_bins(th_context *c, th::DepositParams &p, uint64_t *fragments, bool program = false, const FragmentStage *stage = nullptr);
th_status view_storage(th_context *c);
void view_fields(th_context *c, const th_render_uniforms *u, th::DepositParams &p);
th_status view_params(th_context *c, const th_render_uniforms *u, th::DepositParams &p, bool want_bins = false, bool *bins = nullptr, const FragmentStage *stage = nullptr);
// the binned pipeline in parts (deposit_run_bins = emit + finish; row-band shards put the owners' exchange in between)
constexpr th_status kRetryInStreamOrder = -1;        // (internal) the binned pass gave up before it touched a target
th_status bins_store_for(th_context *c, th::DepositParams &p, uint32_t at_least);
th_status bins_store_grow_keep(th_context *c, th::DepositParams &p, uint32_t pool);
th_status bins_table_widen(th_context *c, th::DepositParams &p, bool keep);       // kRetryInStreamOrder: as wide as it goes (or no memory)
th_status bins_pass_emit(th_context *c, th::DepositParams &p, bool blend_early, bool program = false, const FragmentStage *stage = nullptr);
void bins_pass_expect(th_context *c, th::DepositParams &p);          // before the plan's kernels are launched with p ...
th_status bins_pass_totals(th_context *c, const th::DepositParams &p);  // ... their totals in c->bins_totals_host
th_status bins_pass_finish(th_context *c, th::DepositParams &p, uint64_t *fragments, bool blended_early);
// the flags of an emitting / laying-out attempt that is not worth another one: anything but a dry pool or a full bin, or six attempts
inline bool bins_flags_final(uint32_t flags, int attempt) { return (flags & ~(th::kBinsPoolExhausted | th::kBinsBinFull)) || attempt >= 6; }
bool binned_shards(const th_context *c);              // a sharded draw() of this job goes through the bins (the same answer on every rank)
th_status deposit_prepare_bins(th_context *c, const th_deposit_uniforms *u, th::DepositParams &p);
// what the entry points of a draw say alike
void draw_moves_nothing(th_context *c);               // a local draw: nothing travels between ranks (th_draw_query)
inline void draw_streamed(th_context *c, uint64_t n) { c->last_draw.pipeline = TH_DRAW_STREAM; c->last_draw.fragments = n; c->last_draw.crowded_fragments = 0; }      // (th_draw_query of a stream-ordered pass)
th_status refuse_band(const th_context *c, const char *what, const char *instead);       // TH_OK on a whole texture
th_status shared_uniforms(const th_deposit_uniforms *du, const th_render_uniforms *ru);  // the passes of one draw agree on what they draw
th_deposit_uniforms deposit_uniforms_of(const th_render_uniforms &u);
th_status missing_halo(const th_context *c);          // the error of a band's line that reads a row nobody supplied
// The pass `s` behind its entry point's own checks: drawn on a whole texture through draw_pass - the policy, the bins, the retry -,
// or emitted on a row band (a whole-texture context: the band of all rows) - prepared, its vertex kernel if it has one, emit_parted
th_status pass_run(th_context *c, const PassSpec &s, uint64_t *fragments);
th_status pass_emit(th_context *c, const PassSpec &s, uint64_t *count, void **keys_dev, void **colors_dev);

// ---- th_shard.hip ----------------------------------------------------------------------------------------------------
// the sharded deposit's keys hold 24 texel bits: `target` ("flow", "view") names what is too large for them
th_status texels_fit_keys(const th_context *c, const char *target);
// the tail of every emit of a row band: the fragments of the (prepared) pass `p` - this band's lines - counted, scanned, keyed
// (owner, texel, global stream index), `stage` (or null) over them, parted by owner; synchronises (the caller hands the buffers to a collective)
th_status emit_parted(th_context *c, th::DepositParams &p, const FragmentStage *stage, uint64_t *count, void **keys_dev, void **colors_dev);

// One pass of a local draw: prepare(p, first, &bins) readies `p` for an attempt - the first may take the bins - and says which
// pipeline it takes (with `stage` the bins only under TH_OPT_STAGE_BINS); a binned pass that gives up before blending is repeated in stream order - its stage
// with it, once - and so are the other passes of its frame.
template <class Prepare>
th_status draw_pass(th_context *c, uint64_t *fragments, bool program, const FragmentStage *stage, Prepare prepare)
{
    for (int attempt = 0;; ++attempt) {
        th::DepositParams p;
        bool bins = false;
        if (th_status s = prepare(p, attempt == 0, &bins)) return s;
        if (!bins) return deposit_run(c, p, stage, fragments);
        const th_status s = deposit_run_bins(c, p, fragments, program, stage);
        if (s != kRetryInStreamOrder) return s;
        c->frame_bins = 0;                  // (the other passes of this frame as well)
    }
}

}  // namespace thi
