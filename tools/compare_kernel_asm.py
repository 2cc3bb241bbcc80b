"""Compare the gfx950 device code of two builds of a .hip file kernel by kernel.

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S jvp.hip -o new.s      (the same for the other commit: old.s)
    python tools/compare_kernel_asm.py old.s new.s

Per kernel (mangled symbol): the instruction text between its label and .Lfunc_end, and its .amdhsa_* descriptor block, after
dropping comments and the function index of local labels (it shifts when functions are added or removed).  Exit status 1 when
a kernel both files have differs."""
import re
import sys


def kernels(path):
    text = re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1", open(path).read())
    lines = [re.sub(r"\s*;.*", "", l).rstrip() for l in text.split("\n")]
    lines = [l for l in lines if l.strip()]
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", "\n".join(lines), flags=re.M):
        body = lines[lines.index(name + ":") + 1:]
        body = body[:next(i for i, l in enumerate(body) if l.startswith(".Lfunc_end"))]
        start = lines.index("\t.amdhsa_kernel " + name)
        desc = lines[start:lines.index("\t.end_amdhsa_kernel", start)]
        out[name] = (body, desc)
    return out


def main(old_path, new_path):
    old, new = kernels(old_path), kernels(new_path)
    differ = [k for k in sorted(set(old) & set(new)) if old[k] != new[k]]
    print(f"{len(old)} kernels in {old_path}, {len(new)} in {new_path}, {len(set(old) & set(new))} in both, {len(differ)} differ")
    for title, names in (("only in " + old_path, set(old) - set(new)), ("only in " + new_path, set(new) - set(old)),
                         ("differ", differ)):
        for k in sorted(names):
            print(f"  {title}: {k}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
