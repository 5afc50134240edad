// th_bins_walk.inc - the walk over the page store of a binned pass (th_bins.hip), between its emit and its blends: what the
// library's own kernel that writes a record beside every place (th_fragline.hip: fragment_lines_bins_kernel) and the text put in
// front of a caller's fragment program (th_fragment_prelude.inc: the three bins entry points) must visit alike, place for place -
// the line records lie where the stage's kernel reads them.  ONE copy, read twice, as th_packed.inc.  The includer defines
// TH_BINS_WALK:
//   th_fragline.hip  #define TH_BINS_WALK(...) __VA_ARGS__      the walk itself (its static_assert ties the constants to th_bins.hip's)
//   th_fragprog.hip  #define TH_BINS_WALK(...) #__VA_ARGS__     its text, handed to hiprtc in front of the fragment prelude
// Hence: no preprocessor directive and no project name inside TH_BINS_WALK( ), only what hipcc and hiprtc both know.
//
// Between the emitting pass and the blends every fragment of a binned pass lies at a PLACE of the store: its key
// (y << 44 | x << 32 | stream index of its line; all ones: a place handed out and not written) in keys[place], whatever else
// belongs to it at the same index of the caller's arrays.  A bin is th_bins_replicas lists of pages of 2^th_bins_page_shift
// places; list l = bin * th_bins_replicas + r has handed out the places v < cursor(bin, r), its cursor at
// cursors[r * stride + (bin & 31) * ((nbins + 31) >> 5) + (bin >> 5)]; place v lies in page v >> th_bins_page_shift of the list -
// page 0 is page l of the store, a further page n is page_table[l * max_pages + n] (0: none was published, 0xffffffff: the pool
// was dry) - at v's low bits.
//
// The walk: blockIdx.x is a bin, whose places - its lists one after the other, as bins_blend_kernel walks them - go to the
// workgroup's 256 lanes in rounds; blockIdx.y deals the rounds of one bin to gridDim.y workgroups (a crowded target puts half a
// million fragments into one bin).  The grid is sized by bins, not by fragments: the cursors are on the device.  Skipped: the
// whole pass when it raised a flag or asked for a row nobody holds (it is repeated or abandoned, its table not to be trusted);
// places at or beyond a list's cursor, the cursor clamped to the max_pages pages a list can hold; pages the table does not hold
// (entry 0 or 0xffffffff, page number >= max_pages, an id outside the store); places whose key is the empty key.  body(key, at)
// runs for every other place.  No LDS (a lane's list is found among sixteen running sums the wave holds in scalar registers), no
// atomics, no store of its own.  Both loops over the lists have a constant trip count: the compiler unrolls them without being
// told and first[] never leaves the scalar registers - the same instructions with and without an unroll pragma, which a macro's
// argument could only hold as _Pragma (profiles/fragment_stage_walk.txt).
TH_BINS_WALK(
constexpr unsigned th_bins_replicas = 16u;
constexpr unsigned th_bins_page_shift = 8u;
constexpr int th_bins_tot_oob = 1;
constexpr int th_bins_tot_flags = 2;

struct th_bins_store {
    const unsigned long long *keys;      // per place
    const unsigned *cursors;             // the lists' cursors
    const unsigned *page_table;          // per list max_pages entries
    const unsigned *totals;              // the pass's totals: [th_bins_tot_oob], [th_bins_tot_flags] not 0 - a pass nobody will blend
    unsigned stride, max_pages, nbins;
    unsigned pages;                      // pages of the store: every page id is below it
};

template <class Body>
__device__ __forceinline__ void th_bins_walk(const th_bins_store &s, Body body)
{
    if (s.totals[th_bins_tot_flags] != 0u || s.totals[th_bins_tot_oob] != 0u) return;
    const unsigned b = blockIdx.x;
    if (b >= s.nbins) return;
    const unsigned list_cap = s.max_pages << th_bins_page_shift;
    const unsigned *cursor = s.cursors + (size_t)(b & 31u) * ((s.nbins + 31u) >> 5) + (b >> 5);
    unsigned first[th_bins_replicas + 1u];
    first[0] = 0u;
    for (unsigned r = 0; r < th_bins_replicas; ++r) {
        const unsigned n = cursor[(size_t)r * s.stride];
        first[r + 1u] = first[r] + (n < list_cap ? n : list_cap);
    }
    const unsigned n = first[th_bins_replicas], rounds = (n + 255u) >> 8;
    for (unsigned round = blockIdx.y; round < rounds; round += gridDim.y) {
        const unsigned w = (round << 8) + threadIdx.x;
        if (w >= n) continue;
        unsigned r = 0u, base = 0u;
        for (unsigned q = 1; q < th_bins_replicas; ++q) if (w >= first[q]) { r = q; base = first[q]; }
        const unsigned list = b * th_bins_replicas + r, v = w - base, pn = v >> th_bins_page_shift;
        unsigned id = list;
        if (pn != 0u) {
            if (pn >= s.max_pages) continue;
            id = s.page_table[(size_t)list * s.max_pages + pn];
            if (id == 0u) continue;
        }
        if (id >= s.pages) continue;
        const unsigned at = (id << th_bins_page_shift) | (v & ((1u << th_bins_page_shift) - 1u));
        const unsigned long long key = s.keys[at];
        if (key == ~0ull) continue;
        body(key, at);
    }
}
)
