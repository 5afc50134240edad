"""The one table of program kinds (tendrils_amd/csrc/th_program_kinds.hpp), the part that needs no GPU: a stand-alone host program
(tests/native/program_kinds_check.cc) built with the address and undefined-behaviour sanitizers walks it as the loader does, and
what it prints is held against the preludes: every kind names exactly the extern "C" kernels its prelude files declare, so
program_loaded finds every entry point it asks a module for."""
import glob
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tendrils_amd", "csrc")

# a kind's prelude label -> the files its text is put together from
TEXTS = {"th_fragment_prelude": ("th_fragment_prelude.inc", "th_fragment_pair_prelude.inc")}


def test_every_kind_names_the_kernels_its_prelude_declares(tmp_path):
    exe = str(tmp_path / "program_kinds_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    "-o", exe, os.path.join(ROOT, "tests", "native", "program_kinds_check.cc")], check=True)
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and not ran.stderr, (ran.stdout, ran.stderr)
    named = {}
    for line in ran.stdout.splitlines():
        kind, prelude, kernel = line.split()
        named.setdefault((int(kind), prelude), []).append(kernel)
    assert sorted(kind for kind, _ in named) == list(range(6))
    declared_anywhere = set()
    for (kind, prelude), kernels in named.items():
        declared = []
        for name in TEXTS.get(prelude, (prelude + ".inc",)):
            declared += re.findall(r'^extern "C" __global__ (?:__launch_bounds__\(\d+\) )?void (\w+)\(', open(os.path.join(CSRC, name)).read(), flags=re.M)
        assert sorted(kernels) == sorted(declared), (prelude, kernels, declared)
        declared_anywhere.update(declared)
    in_the_tree = set()
    for path in glob.glob(os.path.join(CSRC, "*_prelude.inc")):
        in_the_tree.update(re.findall(r'^extern "C" __global__ (?:__launch_bounds__\(\d+\) )?void (\w+)\(', open(path).read(), flags=re.M))
    assert in_the_tree == declared_anywhere          # no prelude's kernel is left out of the table
