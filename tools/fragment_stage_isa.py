"""What the fragment stage's kernels compile to, for one or more source trees side by side (no device needed): VGPRs, SGPRs,
scratch bytes, LDS bytes and instruction count of the eight entry points of a fragment program's module - the text
th_fragment_program_compile hands to hiprtc (taps, the page-store walk where the tree has one, prelude, pair prelude, source),
through hiprtc with the library's flags - for the four programs of the build tests, and of fragment_lines_bins_kernel
(th_fragline.hip, hipcc with the Makefile's flags).  profiles/fragment_stage_walk.txt holds a run of it on a commit and its parent.

Usage: python tools/fragment_stage_isa.py TREE [TREE ...] [--keep DIR]     (--keep: the code objects and disassemblies)
"""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
LLVM = "/opt/rocm/llvm/bin"
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "--offload-arch=gfx950"]       # th_program.hip: program_compile
ENTRIES = ("th_fragment_kernel", "th_fragment_band_kernel", "th_fragment_bins_kernel", "th_fragment_line_kernel", "th_fragment_line_band_kernel",
           "th_fragment_line_bins_kernel", "th_fragment_pair_kernel", "th_fragment_pair_bins_kernel")

# the module's text as th_fragprog.hip puts it together: the same includes, printed
TEXT_OF = r"""#include <cstdio>
#define TH_TAPS(...) #__VA_ARGS__
const char kTaps[] =
#include "th_taps.inc"
    ;
#if __has_include("th_bins_walk.inc")
#define TH_BINS_WALK(...) #__VA_ARGS__
const char kBinsWalk[] =
#include "th_bins_walk.inc"
    ;
#else
const char kBinsWalk[] = "";
#endif
const char kPrelude[] =
#include "th_fragment_prelude.inc"
    ;
const char kPairPrelude[] =
#include "th_fragment_pair_prelude.inc"
    ;
int main() { std::printf("%s\n%s\n%s\n%s\n", kTaps, kBinsWalk, kPrelude, kPairPrelude); }
"""


def hiprtc_compile(rtc, text, name):
    prog = C.c_void_p()
    assert rtc.hiprtcCreateProgram(C.byref(prog), text.encode(), name.encode(), 0, None, None) == 0
    opts = (C.c_char_p * len(FLAGS))(*[f.encode() for f in FLAGS])
    status = rtc.hiprtcCompileProgram(prog, len(FLAGS), opts)
    size = C.c_size_t()
    rtc.hiprtcGetProgramLogSize(prog, C.byref(size))
    log = C.create_string_buffer(size.value + 1)
    rtc.hiprtcGetProgramLog(prog, log)
    assert status == 0 and not log.value.strip(b"\0 \n"), log.value.decode()
    assert rtc.hiprtcGetCodeSize(prog, C.byref(size)) == 0
    code = C.create_string_buffer(size.value)
    assert rtc.hiprtcGetCode(prog, code) == 0
    rtc.hiprtcDestroyProgram(C.byref(prog))
    return code.raw


def kernels_of(path):
    """{kernel symbol: dict(vgprs, sgprs, scratch, lds, instructions)} of a gfx950 code object"""
    notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", path], check=True, capture_output=True, text=True).stdout
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        field = lambda key: re.search(r"\.%s:\s*(\S+)" % key, block).group(1)      # noqa: E731
        out[field("name")] = dict(vgprs=int(field("vgpr_count")), sgprs=int(field("sgpr_count")), scratch=int(field("private_segment_fixed_size")),
                                  lds=int(field("group_segment_fixed_size")))
    asm = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", path], check=True, capture_output=True, text=True).stdout
    with open(path + ".s", "w") as f:
        f.write(asm)
    for name, body in re.findall(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^\s*$|\Z)", asm, flags=re.M | re.S):
        if name in out:
            lines = [l for l in body.splitlines() if l.strip() and not l.lstrip().startswith(("s_nop", "s_code_end"))]
            out[name]["instructions"] = len(lines)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trees", nargs="+")
    ap.add_argument("--keep", default=None)
    args = ap.parse_args()
    from test_fragment_program_build import IDENTITY, VIGNETTE
    from test_fragment_program_line_build import ALL_FIELDS, FALLOFF
    programs = dict(IDENTITY=IDENTITY, VIGNETTE=VIGNETTE, FALLOFF=FALLOFF, ALL_FIELDS=ALL_FIELDS)
    rtc = C.CDLL("libhiprtc.so")
    work = args.keep or tempfile.mkdtemp(prefix="fragment_stage_isa_")
    os.makedirs(work, exist_ok=True)
    table = {}                                       # (program, kernel) -> [per tree]
    for index, tree in enumerate(args.trees):
        csrc = os.path.join(os.path.abspath(tree), "tendrils_amd", "csrc")
        exe = os.path.join(work, "text_of_%d" % index)
        with open(exe + ".cc", "w") as f:
            f.write(TEXT_OF)
        subprocess.run(["g++", "-std=c++17", "-I", csrc, "-o", exe, exe + ".cc"], check=True)
        prelude = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
        for name, source in programs.items():
            path = os.path.join(work, "%s_%d.co" % (name, index))
            with open(path, "wb") as f:
                f.write(hiprtc_compile(rtc, prelude + "\n#line 1 \"%s\"\n" % name + source + "\n", "th_fragment_prelude"))
            found = kernels_of(path)
            for kernel in ENTRIES:
                table.setdefault((name, kernel), []).append(found[kernel])
        path = os.path.join(work, "th_fragline_%d.co" % index)
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "-DTH_TESTING=1",
                        "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", path, os.path.join(csrc, "th_fragline.hip")], check=True)
        for symbol, row in kernels_of(path).items():
            if "fragment_lines_bins_kernel" in symbol:
                table.setdefault(("th_fragline.hip", "fragment_lines_bins_kernel"), []).append(row)
    print("trees: " + ", ".join("[%d] %s" % (i, t) for i, t in enumerate(args.trees)))
    print("per tree: VGPRs / SGPRs / scratch bytes / LDS bytes / instructions")
    for (program, kernel), rows in table.items():
        cells = ["%3d /%4d /%2d /%2d /%5d" % (r["vgprs"], r["sgprs"], r["scratch"], r["lds"], r["instructions"]) for r in rows]
        mark = "" if all(r == rows[0] for r in rows) else "   <- differs"
        print("%-16s %-30s %s%s" % (program, kernel, "   |   ".join(cells), mark))
    print("kept in " + work)


if __name__ == "__main__":
    main()
