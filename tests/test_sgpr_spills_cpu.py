"""No SGPR spill reload inside a loop of the headline tile kernels (hipcc cross-compiles here; no GPU needed).

A gfx950 wave has 102 SGPRs.  The LDS-tile gather used to take 214 dwords of scalar arguments by value and keep them
across its particle loop: the compiler parked 190 of them in the lanes of three VGPRs (`v_writelane_b32`) and fetched them
back with `v_readlane_b32`, a vector-ALU instruction each and the most frequent instruction of the loop.  A plain push
is now an instantiation of its own without the hook, and the hook of the folded sort is read from the kernel-argument segment where it is used
(push_sort.hpp); this test keeps the loops of the headline instantiations -- the plain push, the COUNT | SCATTER push and
the deposition -- free of such reloads.  The limit is a condition, not a measurement: 0 inside loops; outside (the
staging before the loop, the epilogue) spills are allowed.

The loops have readlanes of their own (`__shfl`, `readfirstlane`), so a reload is told by its source: one of the VGPRs
that the function's `v_writelane_b32` spill stores write.  A loop is a cycle of the function's control-flow graph."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# order 3, Galerkin gather, Boris, PushPX, every tile; the plain push and the one that carries the sort's hook (-1: the
# hook names the mode, COUNT | SCATTER in the headline's cycle)
GATHER_PLAIN = "_ZN3wxa23gather_push_tile_kernelILi3ELi1ELi0ELb1ELi0ELi0EEE"
GATHER_SORT = "_ZN3wxa23gather_push_tile_kernelILi3ELi1ELi0ELb1ELi0ELin1EEE"
# order 3, Esirkepov, RowsCfg<768, 3, double, 0, 0>
DEPOSIT = "_ZN3wxa24deposit_tile_rows_kernelILi3ELi1ENS_7RowsCfgILi768ELi3EdLi0ELi0EEEEE"


def kernel_bodies(asm):
    """{symbol: [lines]} of every function of an assembly listing (label to .Lfunc_end)"""
    out, cur, name = {}, None, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            name, cur = m.group(1), []
        elif cur is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = cur
                cur = None
            else:
                cur.append(line)
    return out


def blocks_in_loops(lines):
    """per line: does its basic block lie on a cycle of the function's control-flow graph?  Blocks are cut at the .LBB
    labels; edges are the branches and the fall-through of a block that does not end in s_branch / s_endpgm.  (The layout
    alone does not tell: the compiler places cold blocks behind the function's end and branches back from them.)"""
    blocks = [["", 0, len(lines)]]
    for n, l in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            blocks[-1][2] = n
            blocks.append([m.group(1), n, len(lines)])
    index_of = {b[0]: i for i, b in enumerate(blocks)}
    succ = []
    for i, (_, a, b) in enumerate(blocks):
        out, falls = [], True
        for l in lines[a:b]:
            m = re.match(r"\s*s_(c?)branch\w*\s+(\.LBB\d+_\d+)", l)
            if m:
                out.append(index_of[m.group(2)])
                falls = bool(m.group(1))
            elif re.match(r"\s*s_endpgm", l):
                falls = False
        if falls and i + 1 < len(blocks):
            out.append(i + 1)
        succ.append(out)
    # strongly connected components (Tarjan, iterative): a block is in a loop if its component has another block or
    # it branches to itself
    n = len(blocks)
    index, low, on_stack, stack, cyclic, counter = [None] * n, [0] * n, [False] * n, [], [False] * n, 0
    for root in range(n):
        if index[root] is not None:
            continue
        work = [(root, 0)]
        while work:
            v, k0 = work.pop()
            if k0 == 0:
                index[v] = low[v] = counter
                counter += 1
                stack.append(v)
                on_stack[v] = True
            descended = False
            for k in range(k0, len(succ[v])):
                w = succ[v][k]
                if index[w] is None:
                    work.append((v, k + 1))
                    work.append((w, 0))
                    descended = True
                    break
                if on_stack[w]:
                    low[v] = min(low[v], index[w])
            if descended:
                continue
            if low[v] == index[v]:
                members = []
                while True:
                    w = stack.pop()
                    on_stack[w] = False
                    members.append(w)
                    if w == v:
                        break
                for w in members:
                    cyclic[w] = len(members) > 1 or v in succ[v]
            if work:
                low[work[-1][0]] = min(low[work[-1][0]], low[v])
    in_loop = [False] * len(lines)
    for i, (_, a, b) in enumerate(blocks):
        if cyclic[i]:
            in_loop[a:b] = [True] * (b - a)
    return in_loop


def spill_reloads(lines):
    """(reloads in the function, reloads inside a loop): v_readlane_b32 from a VGPR that v_writelane_b32 stores write"""
    spill_vgprs = {m.group(1) for m in (re.match(r"\s*v_writelane_b32 (v\d+), s\d+, \d+", l) for l in lines) if m}
    in_loop = blocks_in_loops(lines)
    total = inside = 0
    for n, l in enumerate(lines):
        m = re.match(r"\s*v_readlane_b32 s\d+, (v\d+), \d+", l)
        if m and m.group(1) in spill_vgprs:
            total += 1
            inside += in_loop[n]
    return total, inside


def test_the_detector_tells_spill_reloads_from_other_readlanes_and_loops_from_layout():
    asm = ("_ZN3wxa1kEv:\n\tv_writelane_b32 v127, s4, 0\n\tv_readlane_b32 s9, v127, 0\n\ts_cbranch_scc1 .LBB0_4\n"
           ".LBB0_1:\n\tv_readlane_b32 s4, v127, 0\n\tv_readlane_b32 s5, v3, 0\n\tv_readfirstlane_b32 s6, v2\n"
           "\ts_cbranch_vccnz .LBB0_1\n.LBB0_2:\n\tv_readlane_b32 s8, v127, 0\n\ts_cbranch_execz .LBB0_3\n.LBB0_3:\n\ts_endpgm\n"
           ".LBB0_4:\n\tv_readlane_b32 s8, v127, 1\n\ts_branch .LBB0_2\n.Lfunc_end0:\n")   # a cold block that branches back: no loop
    assert spill_reloads(kernel_bodies(asm)["_ZN3wxa1kEv"]) == (4, 1)


def _asm(tmp_path, src):
    out = tmp_path / (src + ".s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "--cuda-device-only", "-S",
           os.path.join(ROOT, "warpx_amd", "csrc", src), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("src,prefixes", [("gather_tile.hip", [GATHER_PLAIN, GATHER_SORT]), ("deposit_tile.hip", [DEPOSIT])])
def test_no_sgpr_spill_reload_in_the_loops_of_the_headline_kernels(tmp_path, src, prefixes):
    bodies = kernel_bodies(_asm(tmp_path, src))
    for prefix in prefixes:
        names = [n for n in bodies if n.startswith(prefix)]
        assert len(names) == 1, (prefix, names)
        total, inside = spill_reloads(bodies[names[0]])
        print(f"{names[0][:80]}: {total} SGPR spill reloads, {inside} inside loops")
        assert inside == 0, (names[0], total, inside)
