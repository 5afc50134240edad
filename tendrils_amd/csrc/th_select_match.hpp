// th_select_match.hpp - the predicate of the built-in passes that ask WHICH particles (th_select.hip, th_histogram.hip): the
// clauses of th_select_uniforms as a kernel carries them, the one predicate both units evaluate, and the checks of the block on
// the host.  The header's words (include/tendrils_hip.h "select").  The slot it is evaluated on is th_ring.hpp's.
#pragma once
#include "th_ring.hpp"

namespace thi {

constexpr uint32_t kSelectFlags = TH_SELECT_BOX | TH_SELECT_SPEED | TH_SELECT_INERT;

// th_select_uniforms as a kernel's argument, and what places a local texel in the whole texture
struct SelectClauses {
    float x0, y0, x1, y1, lo, hi;
    uint32_t stride, phase, flags;
    uint32_t width, row0;             // the texture's width; the band's first row
};

// the clauses of the header, in its words: local texel t of a live-or-admitted particle with state s
TH_D bool select_match(const SelectClauses &p, v4f s, bool live, uint32_t t)
{
    bool m = live || (p.flags & TH_SELECT_INERT);
    if (p.flags & TH_SELECT_BOX) m = m && s.x >= p.x0 && s.x < p.x1 && s.y >= p.y0 && s.y < p.y1;      // (a NaN position fails)
    if (p.flags & TH_SELECT_SPEED) {
        const float q = (s.z * s.z) + (s.w * s.w);
        m = m && q >= p.lo && q <= p.hi;                        // (a NaN q fails)
    }
    if (p.stride > 1u) m = m && (t + p.row0 * p.width) % p.stride == p.phase;
    return m;
}

inline SelectClauses select_clauses(const th_context *c, const th_select_uniforms *u)
{
    SelectClauses q{};
    q.x0 = u->box[0]; q.y0 = u->box[1]; q.x1 = u->box[2]; q.y1 = u->box[3];
    q.lo = u->speed2[0]; q.hi = u->speed2[1];
    q.stride = u->stride; q.phase = u->phase; q.flags = u->flags;
    q.width = (uint32_t)c->cfg.width; q.row0 = (uint32_t)c->cfg.row0;
    return q;
}

// what every entry point that takes a th_select_uniforms refuses, under its own name
inline th_status select_checks(th_context *c, const th_select_uniforms *u, int32_t buffer, const char *entry)
{
    TH_REQUIRE(c, "%s: null context", entry);
    TH_REQUIRE(u, "%s: null uniforms", entry);
    TH_RING_BUFFER_OK(c, buffer, entry);
    TH_REQUIRE(u->stride >= 1u && u->phase < u->stride, "%s: stride %u, phase %u (stride >= 1, phase < stride)", entry, u->stride, u->phase);
    TH_REQUIRE(!(u->flags & ~kSelectFlags), "%s: flags 0x%x (TH_SELECT_BOX | _SPEED | _INERT)", entry, u->flags);
    TH_REQUIRE(u->reserved == 0u, "%s: reserved is %u, not 0", entry, u->reserved);
    if (u->flags & TH_SELECT_BOX)
        TH_REQUIRE(!(std::isnan(u->box[0]) || std::isnan(u->box[1]) || std::isnan(u->box[2]) || std::isnan(u->box[3])), "%s: a NaN in the box", entry);
    if (u->flags & TH_SELECT_SPEED) TH_REQUIRE(!(std::isnan(u->speed2[0]) || std::isnan(u->speed2[1])), "%s: a NaN in speed2", entry);
    TH_RING_TEXELS_OK(c, entry);
    return TH_OK;
}

}  // namespace thi
