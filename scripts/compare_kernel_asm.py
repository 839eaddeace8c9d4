r"""Compare the machine code of every kernel between two sets of gfx950 device assemblies (a source refactor
must leave each kernel's instructions as they were).

    python scripts/compare_kernel_asm.py OLD.s [OLD2.s ...] --new NEW.s [NEW2.s ...] [--rename REGEX=REPL ...] [-v]

The .s files are device-only assemblies, one per source file, made with build.py's flags:

    hipcc --offload-arch=gfx950 <build.py flags> --cuda-device-only -S -o FILE.s csrc/FILE.hip

Kernels are matched by demangled name with namespace qualifiers removed.  A body runs from the kernel's
label to its .Lfunc_end; before the comparison ';' comments and blank lines are dropped, the per-file
function index in .LBB<n>_ and .Lfunc_end<n> is removed, and mangled names inside a body (a kernel that
names itself or a device global) are reduced in the same way as the kernel names.  --rename REGEX=REPL
(re.sub, may be repeated, applied in order) rewrites the OLD side's plain names (of the kernels and inside their bodies), so that a kernel the refactor
renamed is paired with its successor, e.g.

    --rename 'backproject_kernel<(-?\d+), (\w+)>\(BpArgs\)=gather_kernel<\1, \2, 0, 1>(GatherArgs)'

Prints the kernels
only one side has and those whose bodies differ (-v: a unified diff of each); exit status 1 if any.
"""
import difflib
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return out.split("\n")[:len(names)]


def strip_ns(name):
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    return re.sub(r"\bnlosgr::detail::|\bnlosgr::", "", name)


def kernels(path):
    """{plain name: normalised body lines} of every .amdhsa_kernel of an assembly file"""
    text = open(path).read()
    syms = re.findall(r"^\s*\.amdhsa_kernel (\S+)$", text, re.M)
    plain = [strip_ns(d) for d in demangle(syms)]
    lines = text.split("\n")
    start = {}
    for i, ln in enumerate(lines):
        m = re.match(r"(\w+):", ln)   # "symbol:   ; @symbol"
        if m:
            start[m.group(1)] = i
    mangled = sorted(set(re.findall(r"\b_Z\w+", text)), key=len, reverse=True)
    short = dict(zip(mangled, (strip_ns(d) for d in demangle(mangled)))) if mangled else {}
    out = {}
    for sym, name in zip(syms, plain):
        body = []
        for ln in lines[start[sym] + 1:]:
            if re.match(r"\.Lfunc_end\d+:", ln):
                break
            ln = ln.split(";")[0].rstrip()
            if not ln.strip():
                continue
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
            ln = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", ln)
            ln = re.sub(r"\b_Z\w+", lambda m: short.get(m.group(0), m.group(0)), ln)
            body.append(ln)
        assert name not in out or out[name] == body, f"{path}: two kernels named {name}"
        out[name] = body
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "-v"]
    verbose = "-v" in sys.argv[1:]
    renames = []
    while "--rename" in args:
        i = args.index("--rename")
        rx, _, repl = args[i + 1].partition("=")
        renames.append((re.compile(rx), repl))
        del args[i:i + 2]
    if "--new" not in args:
        sys.exit(__doc__)
    cut = args.index("--new")
    old, new = {}, {}
    for p in args[:cut]:
        for name, body in kernels(p).items():
            for rx, repl in renames:    # the body names its kernel too (descriptor, section)
                name, body = rx.sub(repl, name), [rx.sub(repl, ln) for ln in body]
            assert name not in old or old[name] == body, f"{p}: two old kernels named {name}"
            old[name] = body
    for p in args[cut + 1:]:
        for name, body in kernels(p).items():
            # a template kernel of a shared header may be emitted by several files: the copies must agree
            assert name not in new or new[name] == body, f"{p}: {name} differs from another new file's copy"
            new[name] = body
    missing = sorted(set(old) - set(new))
    added = sorted(set(new) - set(old))
    differ = sorted(n for n in old if n in new and old[n] != new[n])
    print(f"{len(old)} kernels before, {len(new)} after: {len(old) - len(missing) - len(differ)} identical, "
          f"{len(differ)} differ, {len(missing)} missing, {len(added)} new")
    for n in missing:
        print("missing:", n)
    for n in added:
        print("new:", n)
    for n in differ:
        print("differs:", n)
        if verbose:
            for ln in difflib.unified_diff(old[n], new[n], "before", "after", lineterm="", n=2):
                print("   ", ln)
    sys.exit(1 if missing or added or differ else 0)


if __name__ == "__main__":
    main()
