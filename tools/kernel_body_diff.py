#!/usr/bin/env python3
"""Compare the gfx950 kernel bodies inside two builds of libnrc_hpm.so, kernel by kernel (llvm-objdump -d of the embedded code objects).

    python tools/kernel_body_diff.py OLD.so NEW.so [--rename FROM=TO ...] [--diff] [name-substring ...]

--rename pairs a kernel whose name changed: OLD.so's kernel FROM is compared with NEW.so's kernel TO, each named by the end of its demangled
name without "(anonymous namespace)::" and without the parameter list, for example
--rename 'k_deep_aov<nrc::RayList>=k_ray_aov<nrc::RayList, nrc::DeepOut>'.  --diff prints the unified diff of every kernel that differs.
Prints, for every kernel both libraries hold (by demangled name; or only those whose name contains one of the substrings), whether the instruction
streams are identical; kernels only one side holds are listed.  What depends on where a kernel lies inside its code object is stripped
before the comparison: addresses, branch-target labels, the pc-relative offsets of the two additions behind an s_getpc_b64 (the address
of a __device__ variable) and the padding behind the last s_endpgm.  Exit status 1 when a common kernel differs.
What a pull request quotes when it claims that a path it did not mean to touch is unchanged."""
import difflib
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def kernel_bodies(lib, tmp, tag):
    so = os.path.join(tmp, tag + ".so")
    shutil.copy(lib, so)
    subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = {}
    for co in sorted(glob.glob(so + ".*gfx950")):
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n(?=[0-9a-f]{16} <[^>]+>:)", dis):
            m = re.match(r"[0-9a-f]{16} <([^>]+)>:", block)
            if not m:
                continue
            lines = []
            pc_relative = 0
            for ln in block.splitlines()[1:]:
                ln = re.sub(r"//.*$", "", ln)                    # address + encoding comment
                ln = re.sub(r"<[^>]+>", "<label>", ln).strip()    # branch targets by label
                if not ln:
                    continue
                if pc_relative and re.match(r"s_addc?_u32 ", ln):
                    ln = re.sub(r"0x[0-9a-f]+$", "<offset>", ln)
                    pc_relative -= 1
                if ln.startswith("s_getpc_b64"):
                    pc_relative = 2
                lines.append(ln)
            while lines and not lines[-1].startswith("s_endpgm"):      # alignment padding in front of the next symbol
                lines.pop()
            out[m.group(1)] = lines
    # by demangled name: a template that gained a trailing parameter pack keeps the name of its instantiation with the pack empty
    names = list(out)
    plain = subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout.split("\n")
    return {re.sub(r"^void ", "", d.strip()).replace("<>(", "("): out[n] for n, d in zip(names, plain)}


def main():
    args, renames, show = [], [], False
    argv = sys.argv[1:]
    while argv:
        arg = argv.pop(0)
        if arg == "--rename":
            renames.append(argv.pop(0))
        elif arg == "--diff":
            show = True
        else:
            args.append(arg)
    old, new, want = args[0], args[1], args[2:]
    with tempfile.TemporaryDirectory() as tmp:
        a, b = kernel_bodies(old, tmp, "old"), kernel_bodies(new, tmp, "new")
    short = lambda n: n.replace("(anonymous namespace)::", "").split("(")[0]      # noqa: E731
    for r in renames:      # OLD's kernel FROM is compared under the full name of NEW's kernel TO
        frm, to = r.split("=", 1)
        was, now = [n for n in a if short(n).endswith(frm)], [n for n in b if short(n).endswith(to)]
        if len(was) != 1 or len(now) != 1:
            sys.exit("--rename %s: %d kernels of %s and %d of %s are named so" % (r, len(was), old, len(now), new))
        a[now[0]] = a.pop(was[0])
    keep = lambda n: not want or any(w in n for w in want)      # noqa: E731
    same = differ = 0
    for name in sorted(set(a) & set(b)):
        if not keep(name):
            continue
        if a[name] == b[name]:
            same += 1
            print("identical  %5d instructions  %s" % (len(a[name]), name))
        else:
            differ += 1
            print("DIFFERENT  %5d -> %5d instructions  %s" % (len(a[name]), len(b[name]), name))
            if show:
                print("\n".join(difflib.unified_diff(a[name], b[name], "old", "new", n=2, lineterm="")))
    for name in sorted(set(a) - set(b)):
        if keep(name):
            print("only in old  %s" % name)
    for name in sorted(set(b) - set(a)):
        if keep(name):
            print("only in new  %s" % name)
    print("%d identical, %d different" % (same, differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
