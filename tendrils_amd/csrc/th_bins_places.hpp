// th_bins_places.hpp - where a fragment of a binned pass lies (th_bins.hip): the arithmetic of the lists' cursors, their pages and
// the places inside them, and the slot walk of the emitting pass - what th_bins.hip's kernels and the kernels that read the page
// store between the emit and the blends (th_fragline.hip: the line records of a binned pass) share.  Moved here from th_bins.hip's
// unnamed namespace word for word: every unit that includes this compiles the text th_bins.hip compiled before.
#pragma once
#include "th_kernels.hpp"
#include "th_math.hpp"

namespace th {
namespace {

constexpr uint32_t kPageShift = 8;
static_assert(kBinPage == 1u << kPageShift, "page size");
constexpr uint32_t kNoPlace = 0xffffffffu;
constexpr uint32_t kPageSpins = 1u << 19;        // tries of page_of<WAIT> (each a sleep of ~128 cycles and a load: ~50 ms in all) before it gives up

TH_D void bins_flag(const DepositParams &p, uint32_t what) { atomicOr(&p.totals[kTotFlags], what); }

// ---- pages ---------------------------------------------------------------------------------------------------------------
// Place `v` (a virtual index handed out by the list's cursor) of list `list` = bin * kBinReplicas + r -> position in the
// key / varying arrays.  The page a place lies in was taken from the pool by whoever's reservation contained the page's
// FIRST place - a thread that had moved the cursor before this one and publishes the page right after, without waiting for
// anybody: the wait below always ends.  Should that ever not hold (a reservation lost, a table entry overwritten), the wait
// gives up after kPageSpins tries - tens of milliseconds, a thousand times the longest wait a pass has been seen to make -:
// the place is nowhere, the pass is flagged (kBinsWaitBroken) and the host repeats the draw in stream order like any pass
// it cannot trust, instead of a launch that never ends.
// (WAIT: inside the pass that hands the pages out - a relaxed device-scope load per try: only the entry's own value is
// needed, nothing else is published with it, and an acquire would empty the caches at every fragment; readers of later
// launches load plainly)
template <bool WAIT>
TH_D uint32_t page_of(const DepositParams &p, uint32_t list, uint32_t pn)
{
    if (pn == 0u) return list;
    if (pn >= p.max_pages) return kNoPlace;
    uint32_t *slot = &p.page_table[(size_t)list * p.max_pages + pn];
    if constexpr (!WAIT) return *slot;
    uint32_t id = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint32_t spins = 0; id == 0u; ++spins) {
        if (spins >= kPageSpins) { bins_flag(p, kBinsWaitBroken); return kNoPlace; }
        __builtin_amdgcn_s_sleep(2);
        id = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return id;                                      // (kNoPlace: the pool was exhausted - flagged by the allocator)
}
template <bool WAIT = false>
TH_D uint32_t place_of(const DepositParams &p, uint32_t list, uint32_t v)
{
    const uint32_t id = page_of<WAIT>(p, list, v >> kPageShift);
    return id == kNoPlace ? kNoPlace : (id << kPageShift) | (v & (kBinPage - 1u));
}
// (the cursors of one list index r, transposed in 32 columns: neighbouring bins' cursors 1 KB apart, not in one 128-byte line -
// the lines that take their places one by one, bins_listed_kernel, meet neighbouring bins at the same time: 50 -> 44 us)
TH_D uint32_t *list_cursor(const DepositParams &p, uint32_t bin, uint32_t r)
{
    return p.bin_cursor + (size_t)r * p.bin_stride + (bin & 31u) * ((p.nbins + 31u) >> 5) + (bin >> 5);
}

// slot s: its particle's texel (col, row) and whether draw() can make a line of it at all (th_api.hip: line_rows)
// (PROGRAM, here and in the kernels that set a line up: a caller's vertex stage has run - th_drawprog.hip - and left
// its vertices in p.vertices, texel-indexed.  Nothing of such a line is read from the ring, so the pass walks the records in
// TEXEL order whatever order the ring is held in - s is the particle's id - and the word `perm` shares with `vertices` is never
// read as a table; <false> is the library's own stage, the text it was)
template <bool PROGRAM = false>
TH_D bool slot_particle(const DepositParams &p, uint32_t s, uint32_t &col, uint32_t &row)
{
    uint32_t pid = s;
    if constexpr (!PROGRAM) pid = p.perm ? p.perm[s] : s;
    if ((p.W & (p.W - 1u)) == 0u) { row = pid >> (31 - __builtin_clz(p.W)); col = pid & (p.W - 1u); }       // (uniform branch)
    else { row = pid / p.W; col = pid - row * p.W; }
    const uint32_t g = p.row0 + row;
    return (p.row_draws[g >> 5] >> (g & 31u)) & 1u;
}

}  // namespace
}  // namespace th
