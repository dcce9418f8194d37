"""Device code of two source trees, compared function by function (no GPU needed):
    python scripts/device_code_diff.py OTHER_TREE [THIS_TREE] > profiles/roundN/device_code_diff.md
For a change that must leave the device side alone (a host-side refactor).  Emits the gfx950 assembly of the four kernel
files of each tree with the flags tests/test_isa_cpu.py uses, cuts it at the function labels and compares the instruction
streams.  The order of the functions in a file follows the order of instantiation, and with it the numbers of the block
labels; a function's own mangled name recurs inside its range and changes where a parameter type is renamed: both are
normalised, and functions are matched by demangled name without the parameter list.
Exit status 1 when a function is missing on one side or differs."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

FILES = [("fields", ["-ffp-contract=off"]), ("particles", []), ("deposit_tile", []), ("gather_tile", [])]
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
    jobs = [(t, n, e) for n, e in FILES for t in (other, this)]
    with ThreadPoolExecutor(max_workers=4) as ex:
        asm = list(ex.map(lambda j: functions(assembly(*j)), jobs))
    bad = 0
    print("# Device code, function by function\n\n`hipcc " + " ".join(FLAGS) + "` on both trees (scripts/device_code_diff.py): "
          "compiler output, not a measurement.\n\n| file | functions, other tree | functions, this tree | equal | differ | only in one |\n"
          "|---|---|---|---|---|---|")
    notes = []
    for i, (name, _) in enumerate(FILES):
        a, b = asm[2 * i], asm[2 * i + 1]
        lone = sorted(set(a) ^ set(b))
        differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
        print(f"| {name}.hip | {len(a)} | {len(b)} | {len(set(a) & set(b)) - len(differ)} | {len(differ)} | {len(lone)} |")
        notes += [f"* {name}.hip differs: `{k}`" for k in differ] + [f"* {name}.hip, only in one tree: `{k}`" for k in lone]
        bad += len(lone) + len(differ)
    if notes:
        print("\n" + "\n".join(notes))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
