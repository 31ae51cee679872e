#!/usr/bin/env python3
"""Is the device code of two source trees the same bytes?  tools/device_asm_diff.py TREE_A TREE_B
Compiles every blom_amd/csrc/*.hip of both trees to gfx950 assembly with the FLAGS of TREE_A's csrc/Makefile (device side only, a fixed
-cuid so that the one symbol hipcc derives from a random number is the same in every run) and prints the files whose assembly differs.
The check for a refactor that must not touch the kernels; it looks at nothing inside the assembly."""
import concurrent.futures, filecmp, glob, os, re, subprocess, sys, tempfile


def flags(tree):
    mk = open(os.path.join(tree, "blom_amd/csrc/Makefile")).read().replace("\\\n", " ")
    f = re.search(r"^FLAGS\s*:=(.*)$", mk, re.M).group(1)
    return f.replace("$(ARCH)", os.environ.get("ARCH", "gfx950")).replace("$(EXTRA)", "").split()


def assemble(job):
    csrc, name, out, fl = job
    r = subprocess.run([os.environ.get("HIPCC", "hipcc")] + fl + ["-cuid=blom", "--cuda-device-only", "-S", name, "-o", out],
                       cwd=csrc, capture_output=True, text=True)
    return r.stderr if r.returncode else None


def main(a, b):
    with tempfile.TemporaryDirectory(prefix="asmdiff") as tmp:
        fl, jobs, names = flags(a), [], set()
        for side, tree in (("a", a), ("b", b)):
            csrc = os.path.join(os.path.abspath(tree), "blom_amd/csrc")
            os.makedirs(os.path.join(tmp, side))
            for p in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
                names.add(os.path.basename(p))
                jobs.append((csrc, os.path.basename(p), os.path.join(tmp, side, os.path.basename(p)[:-4] + ".s"), fl))
        with concurrent.futures.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
            errs = [e for e in ex.map(assemble, jobs) if e]
        if errs:
            sys.exit("\n".join(errs))
        pair = lambda n: [os.path.join(tmp, s, n[:-4] + ".s") for s in "ab"]
        diff = [n for n in sorted(names) if not all(map(os.path.exists, pair(n))) or not filecmp.cmp(*pair(n), shallow=False)]
    print("\n".join("DIFFERS " + n for n in diff) or "%d translation units, device assembly identical" % len(names))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
