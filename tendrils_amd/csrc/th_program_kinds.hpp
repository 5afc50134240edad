// th_program_kinds.hpp - the kinds of caller's program and the entry points of each kind's module: ONE table, which the compile
// (the label of the text hiprtc is given), the error messages, the loader (th_program.hip: program_loaded takes every name of the
// kind from the module) and the launches (ProgramModule::entry, indexed by the kind's enumerators below) all read.  Plain C++:
// nothing of the runtime is named here.
#pragma once

namespace thi {

enum ProgramKind { kStateProgram = 0, kScreenProgram = 1, kDrawProgram = 2, kStepProgram = 3, kFragmentProgram = 4, kMeasureProgram = 5, kProgramKinds = 6 };

// a module's entry points, per kind, in the order of the kind's row: [0] is the kernel th_program_query reports
enum StateEntry { kStateRun };
enum ScreenEntry { kScreenRun };
enum DrawEntry {
    kDrawVertex,                 // the vertex stage over the lines in texel order
    kDrawSlots,                  // ... over a slot order (the binned pipeline)
    kDrawBand,                   // ... of a row band's lines
};
enum StepEntry {
    kStepF32,                    // the fused steps on 16-byte texels
    kStepPacked,                 // ... on a packed ring's 8-byte texels
};
enum FragmentEntry {
    kFragmentStream,             // the fragments of a stream-ordered pass, under 32-bit texel keys
    kFragmentBand,               // ... of an emit, under their 64-bit keys
    kFragmentBins,               // ... of a binned pass, where they lie in the page store
    kFragmentLine,               // kFragmentStream, kFragmentBand, kFragmentBins with the line records behind their record: a
    kFragmentLineBand,           // program that reads th_line
    kFragmentLineBins,
    kFragmentPair,               // kFragmentStream, kFragmentBins over one half of the two varyings a fragment of
    kFragmentPairBins,           // th_draw_stages_pair's one rasterisation carries
};
enum MeasureEntry {
    kMeasureF32,                 // the reduction over 16-byte texels
    kMeasurePacked,              // ... over a packed ring's 8-byte texels
};
constexpr int kMaxProgramEntries = 8;

struct ProgramKindInfo {
    const char *prelude;                         // what hiprtc calls the text in front of the caller's
    const char *what;                            // the kind, as an error message names it
    int entries;
    const char *entry[kMaxProgramEntries];       // the extern "C" kernels of the kind's prelude
};
inline constexpr ProgramKindInfo kProgramKindTable[kProgramKinds] = {
    {"th_program_prelude", "state program (th_program_compile)", kStateRun + 1, {"th_program_kernel"}},
    {"th_screen_prelude", "screen program (th_screen_program_compile)", kScreenRun + 1, {"th_screen_kernel"}},
    {"th_draw_prelude", "draw program (th_draw_program_compile)", kDrawBand + 1, {"th_draw_vertex_kernel", "th_draw_vertex_slots_kernel", "th_draw_vertex_band_kernel"}},
    {"th_step_prelude", "step program (th_step_program_compile)", kStepPacked + 1, {"th_step_kernel", "th_step_packed_kernel"}},
    {"th_fragment_prelude", "fragment program (th_fragment_program_compile)", kFragmentPairBins + 1,
     {"th_fragment_kernel", "th_fragment_band_kernel", "th_fragment_bins_kernel", "th_fragment_line_kernel", "th_fragment_line_band_kernel", "th_fragment_line_bins_kernel",
      "th_fragment_pair_kernel", "th_fragment_pair_bins_kernel"}},
    {"th_measure_prelude", "measure program (th_measure_program_compile)", kMeasurePacked + 1, {"th_measure_kernel", "th_measure_packed_kernel"}},
};
constexpr bool program_kinds_complete()
{
    for (const ProgramKindInfo &k : kProgramKindTable) {
        if (!k.prelude || !k.what || k.entries < 1 || k.entries > kMaxProgramEntries) return false;
        for (int e = 0; e < kMaxProgramEntries; ++e) if ((e < k.entries) != (k.entry[e] != nullptr)) return false;
    }
    return true;
}
static_assert(program_kinds_complete(), "every kind: a label, a description, and exactly as many kernel names as it has enumerators");

}  // namespace thi
