// program_kinds_check.cc - a stand-alone host program over the one table of program kinds (tendrils_amd/csrc/th_program_kinds.hpp),
// for a sanitizer build (tests/test_program_kinds.py: -fsanitize=address,undefined): it walks the table as the loader does - every
// kind, every entry the kind says it has - checks that the kind's enumerators index inside ProgramModule's array and inside the
// kind's own list, and prints "kind prelude kernel" per entry for the test to hold against the preludes' texts.
#include <cstdio>
#include <cstring>

#include "th_program_kinds.hpp"

using namespace thi;

int main()
{
    // the last enumerator of every kind, by kind: what the launches index ProgramModule::entry with
    const int last[kProgramKinds] = {kStateRun, kScreenRun, kDrawBand, kStepPacked, kFragmentPairBins, kMeasurePacked};
    int bad = 0;
    const char *slots[kMaxProgramEntries];      // as ProgramModule::entry is filled
    for (int kind = 0; kind < kProgramKinds; ++kind) {
        const ProgramKindInfo &k = kProgramKindTable[kind];
        if (k.entries < 1 || k.entries > kMaxProgramEntries || last[kind] != k.entries - 1) { std::printf("kind %d: %d entries, last enumerator %d\n", kind, k.entries, last[kind]); ++bad; continue; }
        if (!k.prelude || !*k.prelude || !k.what || !std::strstr(k.what, "_compile")) { std::printf("kind %d: no label or description\n", kind); ++bad; }
        for (int e = 0; e < k.entries; ++e) {
            slots[e] = k.entry[e];
            if (!slots[e] || !*slots[e]) { std::printf("kind %d entry %d: no name\n", kind, e); ++bad; continue; }
            for (int f = 0; f < e; ++f) if (!std::strcmp(slots[f], slots[e])) { std::printf("kind %d: %s twice\n", kind, slots[e]); ++bad; }
            std::printf("%d %s %s\n", kind, k.prelude, slots[e]);
        }
    }
    return bad ? 1 : 0;
}
