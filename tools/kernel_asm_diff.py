"""Is the device code of two source trees the same, kernel by kernel?  (build tooling beside kernel_resources.py; needs hipcc, no GPU)

usage: tools/kernel_asm_diff.py OLD_CSRC [NEW_CSRC] [-DFLAG ...]
OLD_CSRC: the csrc/ of another checkout (``git worktree add ../parent HEAD~1``); NEW_CSRC defaults to this tree's.

Every *.hip of both directories is compiled with build.py's FLAGS (+ that file's EXTRA_FLAGS, + the flags given here) and
--cuda-device-only -S.  The assembly is cut at each kernel symbol, from its label to its .Lfunc_end; comments and .loc / .file /
.cfi lines are dropped and the function index in local labels is replaced.  What is left is compared together with the kernel's
.amdhsa_kernel block (register counts, LDS, scratch), whichever file the kernel lives in.  Prints the kernels per file and every
kernel lost, added or changed; exits 1 if there is any.
"""
import glob
import importlib.util
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = importlib.import_module("ddim_audio_amd.build")  # (as part of its package: it takes the header list from ddim_audio_amd._lib)

DROP = re.compile(r"\s*(;|\.loc\s|\.file\s|\.cfi_)")
LOCAL = re.compile(r"\.(LBB|Ltmp|LJTI|LCPI|Lfunc_begin|Lfunc_end)\d+")
DESC = re.compile(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", re.M | re.S)


def kernels(path, extra):
    """{kernel symbol: (file name, [body lines], descriptor text)} of one translation unit"""
    base = os.path.basename(path)
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + B.FLAGS + B.EXTRA_FLAGS.get(base, []) + extra
    r = subprocess.run(cmd + ["--cuda-device-only", "-S", path, "-o", "-"], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("hipcc failed for %s:\n%s" % (path, r.stderr[-4000:]))
    lines = r.stdout.splitlines()
    out = {}
    for m in DESC.finditer(r.stdout):
        i = next(k for k, l in enumerate(lines) if l.startswith(m.group(1) + ":"))
        j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
        body = [LOCAL.sub(r".\1#", l.split(";")[0].rstrip()) for l in lines[i:j + 1] if not DROP.match(l)]
        out[m.group(1)] = (base, [l for l in body if l], m.group(2))
    return out


def tree(csrc, extra):
    print(csrc)
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")))
    with ThreadPoolExecutor(max_workers=8) as ex:
        units = list(ex.map(lambda f: kernels(f, extra), files))
    merged = {}
    for f, u in zip(files, units):
        print("  %-28s %3d kernels" % (os.path.basename(f), len(u)))
        if set(u) & set(merged):
            sys.exit("defined twice in %s: %s" % (csrc, sorted(set(u) & set(merged))))
        merged.update(u)
    return merged


def main():
    dirs = [a for a in sys.argv[1:] if not a.startswith("-")]
    extra = [a for a in sys.argv[1:] if a.startswith("-")]
    if not 1 <= len(dirs) <= 2:
        sys.exit(__doc__)
    old = tree(dirs[0], extra)
    new = tree(dirs[1] if len(dirs) == 2 else os.path.join(ROOT, "ddim_audio_amd", "csrc"), extra)
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in new or name not in old:
            print("%s %s (%s)" % ("LOST " if name in old else "ADDED", name, (old.get(name) or new.get(name))[0]))
        elif old[name][1:] != new[name][1:]:
            o, n = old[name], new[name]
            print("CHANGED (%s) %s: %s %d lines -> %s %d lines" % ("body" if o[1] != n[1] else "descriptor", name, o[0], len(o[1]),
                                                                 n[0], len(n[1])))
        else:
            continue
        bad += 1
    moved = sum(1 for k in old if k in new and old[k][0] != new[k][0])
    print("%d kernels old, %d new, %d in another file than before, %d lost / added / changed" % (len(old), len(new), moved, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
