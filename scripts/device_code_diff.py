"""Device code of two source trees, compared function by function (no GPU needed):
    python scripts/device_code_diff.py OTHER_TREE [THIS_TREE] > profiles/roundN/device_code_diff.md
For a change that must leave the device side alone (a host-side refactor).  Emits the gfx950 assembly of the kernel
files of each tree with the flags tests/test_isa_cpu.py uses, cuts it at the function labels and compares the instruction
streams.  The order of the functions in a file follows the order of instantiation, and with it the numbers of the block
labels; a function's own mangled name recurs inside its range and changes where a parameter type is renamed: both are
normalised, and functions are matched by demangled name without the parameter list, over all the files of a tree.
Exit status 1 when a function is missing on one side or differs."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

FILES = [("fields", ["-ffp-contract=off"]), ("particles", []), ("inject", []), ("deposit_tile", []), ("gather_tile", [])]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "--cuda-device-only", "-S"]


def assembly(tree, name, extra):
    src = os.path.join(tree, "warpx_amd", "csrc", name + ".hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *extra, src, "-o", "-"], capture_output=True, text=True, cwd="/tmp")
    if r.returncode != 0:
        sys.exit(f"hipcc failed for {src}:\n{r.stderr}")
    return r.stdout


def functions(asm):
    """{demangled name without parameters: normalised text from the label to .Lfunc_end}"""
    out, sym, body, ended = {}, None, [], False

    def close():
        dem = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
        depth, i = 0, dem.rfind(")")
        for j in range(i, -1, -1):   # cut the parameter list: from the last ")" back to its "("
            depth += (dem[j] == ")") - (dem[j] == "(")
            if depth == 0:
                dem = dem[:j]
                break
        while dem in out:   # overloads
            dem += "'"
        out[dem] = "\n".join(body)

    for line in asm.splitlines():
        m = re.match(r"(_Z\w+):", line)
        # the kernel descriptor (.amdhsa_kernel: registers, LDS, scratch) follows .Lfunc_end and belongs to the function;
        # the next function's preamble does not
        if sym and (m or (ended and re.match(r"\s*\.(text|section\s+\.(text|AMDGPU\.gpr_maximums)|protected|globl|weak|hidden|amdgpu_metadata|ident)\b", line))):
            close()
            sym = None
        if m:
            sym, body, ended = m.group(1), [], False
        if sym is None:
            continue
        line = re.sub(r"\s*;.*", "", line).rstrip()
        if line:
            line = re.sub(r"\.LBB\d+_", ".LBB_", line).replace(sym, "SELF")
            body.append(re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", line))
        ended = ended or line.startswith(".Lfunc_end")
    if sym:
        close()
    return out


def main():
    other = os.path.abspath(sys.argv[1])
    this = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # a tree may lack a file of the list (it was split off later): functions are matched over the union of a tree's files,
    # so that one that moved compares against itself
    jobs = [(t, n, e) for n, e in FILES for t in (other, this) if os.path.exists(os.path.join(t, "warpx_amd", "csrc", n + ".hip"))]
    with ThreadPoolExecutor(max_workers=4) as ex:
        asm = list(ex.map(lambda j: functions(assembly(*j)), jobs))
    a, b = {}, {}   # {function: (file, text)}
    for (t, n, _), fns in zip(jobs, asm):
        side = a if t == other else b
        for k, text in fns.items():
            while k in side:   # the same name in two files
                k += "'"
            side[k] = (n, text)
    print("# Device code, function by function\n\n`hipcc " + " ".join(FLAGS) + "` on both trees (scripts/device_code_diff.py): "
          "compiler output, not a measurement.\n\n| file, this tree | functions | equal | of those, in another file of the other tree | differ | only in this tree |\n"
          "|---|---|---|---|---|---|")
    notes = [f"* only in the other tree ({a[k][0]}.hip): `{k}`" for k in sorted(set(a) - set(b))]
    for name, _ in FILES:
        mine = [k for k in b if b[k][0] == name]
        both = [k for k in mine if k in a]
        differ = sorted(k for k in both if a[k][1] != b[k][1])
        moved = [k for k in both if a[k][0] != name and k not in differ]
        print(f"| {name}.hip | {len(mine)} | {len(both) - len(differ)} | {len(moved)} | {len(differ)} | {len(mine) - len(both)} |")
        notes += [f"* {name}.hip differs: `{k}`" + (f" (from {a[k][0]}.hip)" if a[k][0] != name else "") for k in differ]
        notes += [f"* {name}.hip, only in this tree: `{k}`" for k in sorted(set(mine) - set(both))]
    if notes:
        print("\n" + "\n".join(notes))
    return 1 if notes else 0


if __name__ == "__main__":
    sys.exit(main())
