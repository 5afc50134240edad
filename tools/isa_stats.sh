#!/bin/bash
# ISA of one kernel (default: the exact fused integrator over the window tables): registers, scratch, and the VALU count of its
# step loop - hot path plus back-edge block, with the speed clamp's slow block and the cold fallback as separate figures
# (tools/isa_loop_blocks.py says how the blocks are told apart).
#   tools/isa_stats.sh [kernel symbol]        TH_SRC=<another checkout's tendrils_amd/csrc>: count that tree the same way
set -u
HERE=$(cd "$(dirname "$0")" && pwd)
K=${1:-_ZN2th18logic_fused_kernelILb0ELb1ELb0ELb1ELb1ELb1ELb1EEEvNS_11LogicParamsE}
SRC=${TH_SRC:-$HERE/../tendrils_amd/csrc}
OUT=$(mktemp -d)
cd "$SRC" || exit 1
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -DTH_TESTING=1 -I../../include -S --cuda-device-only -o "$OUT/th_kernels.s" th_kernels.hip 2>/dev/null || exit 1
grep -A30 "^\s*.amdhsa_kernel $K" "$OUT/th_kernels.s" | grep -E "next_free_vgpr|next_free_sgpr|private_segment_fixed"
python3 "$HERE/isa_loop_blocks.py" "$OUT/th_kernels.s" "$K"
rm -rf "$OUT"
