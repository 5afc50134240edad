#!/usr/bin/env python3
"""VALU count of a fused kernel's step loop from its assembly listing (tools/isa_stats.sh calls this).

    tools/isa_loop_blocks.py listing.s kernel_symbol

The step loop is the kernel's depth-2 loop.  Its blocks are told by the compiler's own annotations ("Inner Loop Header:
Depth=2", "in Loop: Header=.. Depth=2"), wherever the layout puts them - the compiler lays the back-edge block behind the ~950
lines of the inlined reference-order fallback, or the fallback's tail in front of the header.  The loop is walked from its
header along the branches; what a conditional branch skips (the blocks reachable from its fall-through before its target) is a
conditional region.  The blocks are split into
  hot path     every block a lane inside the domain executes when the speed clamp's slow branch is not taken, the back-edge
               block included
  slow clamp   the conditional region inside the hot path that holds the clamp's sqrt (exact) / rsq (fast)
  cold         the conditional region that holds more than two true divisions (v_div_fixup_f32): the inert / NaN /
               reference-order branch of lanes outside the domain, logic_texel_ref inlined - the hot path divides once, in
               the clamp's slow block; what else it would divide depends on the particle id alone and is hoisted
  last store   a region under a scalar branch that holds a global store: the state before the last step (once per launch)
"""
import collections
import re
import sys


def kernel_lines(path, sym):
    out, on = [], False
    for line in open(path):
        if not on and line.startswith(sym + ":"):
            on = True
        if on:
            out.append(line.rstrip("\n"))
            if line.startswith(".Lfunc_end"):
                break
    return out


def blocks_of(lines):
    """[(name, annotation, [instruction lines])] in layout order"""
    blocks = [("entry", "", [])]
    for line in lines:
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", line) or re.match(r"^; %bb\.(\d+):\s*(;.*)?$", line)
        if m:
            blocks.append((m.group(1), m.group(2) or "", []))
        elif re.match(r"^\s+;\s", line) and not blocks[-1][2]:
            blocks[-1] = (blocks[-1][0], blocks[-1][1] + " " + line.strip(), [])     # ("=> This Inner Loop Header" on a second line)
        elif re.match(r"^\s+[a-z;]", line):
            blocks[-1][2].append(line.strip())
    return blocks


def valu(ins):
    return [i for i in ins if i.startswith("v_")]


def main():
    path, sym = sys.argv[1], sys.argv[2]
    blocks = blocks_of(kernel_lines(path, sym))
    hdr = next((k for k, b in enumerate(blocks) if "Inner Loop Header: Depth=2" in b[1]), None)
    if hdr is None:
        sys.exit("no depth-2 loop in %s" % sym)
    tag = "Header=%s Depth=2" % blocks[hdr][0].lstrip(".L")
    loop = [k for k, b in enumerate(blocks) if k == hdr or tag in b[1]]
    index = {b[0]: k for k, b in enumerate(blocks)}
    in_loop = set(loop)

    def branches(k):
        """(conditional targets inside the loop, the block that follows when none is taken)"""
        conds, nxt = [], k + 1
        for i in blocks[k][2]:
            m = re.match(r"s_cbranch_(\w+)\s+(\.LBB\d+_\d+)", i)
            if m and index.get(m.group(2)) in in_loop:
                conds.append((m.group(1), index[m.group(2)]))
            m = re.match(r"s_branch\s+(\.LBB\d+_\d+)", i)
            if m:
                nxt = index.get(m.group(1))
        return conds, nxt

    def reach(s, stop):
        seen, todo = [], [s]
        while todo:
            k = todo.pop()
            if k is None or k == stop or k == hdr or k not in in_loop or k in seen:
                continue
            seen.append(k)
            conds, nxt = branches(k)
            todo += [t for _, t in conds] + [nxt]
        return sorted(seen)

    def walk(k, stop):
        """the blocks every lane passes from k to stop, and the regions skipped on the way: (kind of branch, blocks, first block)"""
        chain, regions = [], []
        while k is not None and k != stop and k in in_loop and k not in chain:
            chain.append(k)
            conds, nxt = branches(k)
            conds = [c for c in conds if c[1] != hdr]
            if conds:
                kind, t = conds[-1]
                regions.append((kind, reach(nxt, t), nxt))
                k = t
            else:
                k = nxt
            if k == hdr:
                break
        return chain, regions

    def text(ks):
        return [i for k in ks for i in blocks[k][2]]

    hot, regions = walk(hdr, None)
    back = hot[-1:]
    cold, clamp, last = [], [], []
    for kind, r, first in regions:
        if sum(i.startswith("v_div_fixup_f32") for i in text(r)) > 2:
            cold += r
        elif not kind.startswith("exec") and any(i.startswith("global_store") for i in text(r)):
            last += r
        else:
            chain, inner = walk(first, None if not r else max(r) + 1)
            chain = [k for k in chain if k in r]
            hot += chain
            for _, n, _ in inner:
                if any(re.match(r"v_(sqrt|rsq)_f32", i) for i in text(n)) and len(valu(text(n))) <= 64:
                    clamp += n
                else:
                    hot += n
            hot += [k for k in r if k not in hot and k not in clamp]
    hot = sorted(set(hot))

    name = lambda ks: " ".join(blocks[k][0] for k in ks) or "-"
    hot_ins = [i for i in text(hot) if re.match(r"[vsdg][a-z_]", i)]
    hist = collections.Counter(re.sub(r"_e(32|64)$", "", i.split()[0]) for i in hot_ins)
    print("step loop: header %s, %d blocks; hot path: %s" % (blocks[hdr][0], len(loop), name(hot)))
    print("  ".join("%s:%d" % kv for kv in hist.most_common()))
    print("VALU hot path + back edge: %d   (back-edge block %s: %d, of them v_mov_b32: %d)" % (
        len(valu(text(hot))), name(back), len(valu(text(back))), sum(i.startswith("v_mov_b32") for i in text(back))))
    print("VALU slow clamp block (%s): %d" % (name(clamp), len(valu(text(clamp)))))
    print("VALU cold fallback (%s .. %s, %d blocks): %d" % (blocks[cold[0]][0] if cold else "-", blocks[cold[-1]][0] if cold else "-",
                                                           len(cold), len(valu(text(cold)))))
    print("VALU last-step store block, once per launch (%s): %d" % (name(last), len(valu(text(last)))))
    sg = [i for i in valu(text(hot)) if not re.match(r"v_(cndmask|cmp|readfirstlane)", i) and re.search(r", s(\d+|\[)", i)]
    print("VALU with SGPR source (hot path): %d" % len(sg))


if __name__ == "__main__":
    main()
