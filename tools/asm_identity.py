#!/usr/bin/env python3
"""Is the device code of csrc/*.hip files the same as at a git revision?  Needs no GPU.

    python tools/asm_identity.py [--dump DIR] <rev> gemm_frd.hip gemm_fr64.hip ...     (names in ditto_tts_amd/csrc, or paths)

Every file is compiled twice to gfx950 assembly with build.py's FLAGS + EXTRA plus `-S --cuda-device-only`: once from the working
tree, once from <rev>, whose csrc/ and include/ are extracted with `git archive` into a temporary directory.  The two outputs are
normalised (`.file`, `.ident` and every line that names the per-compilation `__hip_cuid_` symbol dropped) and compared per kernel
symbol: instruction count and a hash over the kernel's body AND its `.amdhsa_kernel` descriptor (register counts, LDS, scratch)
for both sides.  Exit status 1 on any difference — a kernel only one side has, a differing hash, or differing text outside the
kernels.  --dump DIR keeps both normalised listings (DIR/<file>.old.s, .new.s) for a diff.  What a refactor of hand-scheduled kernels is held to: the same machine code, not a timing tolerance.
"""
from __future__ import annotations

import hashlib
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ditto_tts_amd.build import EXTRA, FLAGS, HIPCC  # noqa: E402

CSRC_REL, INCLUDE_REL = "ditto_tts_amd/csrc", "include"


def flags_for(root: str) -> list[str]:
    """build.py's FLAGS with its two include directories pointed into `root`."""
    out, it = [], iter(FLAGS)
    for f in it:
        if f == "-I":
            d = next(it)
            out += ["-I", os.path.join(root, os.path.relpath(d, ROOT))]
        else:
            out.append(f)
    return out


def compile_asm(root: str, name: str) -> str:
    src = os.path.join(root, CSRC_REL, name)
    cmd = [HIPCC, *flags_for(root), *EXTRA.get(name, []), "-S", "--cuda-device-only", src, "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{r.stderr}")
    return r.stdout


def normalise(text: str) -> list[str]:
    return [ln.rstrip() for ln in text.splitlines()
            if not re.match(r"\s*\.(file|ident)\b", ln) and "__hip_cuid_" not in ln]


def split_kernels(lines: list[str]):
    """-> ({kernel: (instruction count, hash of body + descriptor)}, hash of everything else)"""
    names = [m.group(1) for ln in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))]
    parts: dict[str, list[str]] = {n: [] for n in names}
    ninstr = {n: 0 for n in names}
    rest: list[str] = []
    cur = None          # kernel whose body or descriptor the line belongs to
    for ln in lines:
        if cur is None:
            m = re.match(r"(\S+):", ln)
            if m and m.group(1) in parts:
                cur = m.group(1)
            elif (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)):
                cur = m.group(1)
        if cur is None:
            rest.append(ln)
            continue
        parts[cur].append(ln)
        s = ln.strip()
        if ln[:1] in "\t " and s and s[0] not in ".;" and not s.endswith(":"):
            ninstr[cur] += 1
        if re.match(r"\.Lfunc_end\d+:", s) or s == ".end_amdhsa_kernel":
            cur = None
    h = lambda ls: hashlib.sha256("\n".join(ls).encode()).hexdigest()[:16]
    return {n: (ninstr[n], h(parts[n])) for n in names}, h(rest)


def demangled(names: list[str]) -> dict[str, str]:
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(argv: list[str]) -> int:
    dump = None
    if len(argv) > 2 and argv[1] == "--dump":
        dump = argv[2]
        os.makedirs(dump, exist_ok=True)
        argv = argv[:1] + argv[3:]
    if len(argv) < 3:
        print(__doc__)
        return 2
    rev, files = argv[1], [os.path.basename(f) for f in argv[2:]]
    sha = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", rev], capture_output=True, text=True, check=True).stdout.strip()
    ndiff = nkern = 0
    with tempfile.TemporaryDirectory() as old:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC_REL, INCLUDE_REL], capture_output=True, check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(old)
        present = [f for f in files if os.path.exists(os.path.join(old, CSRC_REL, f))]
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            new_asm = dict(zip(files, ex.map(lambda f: compile_asm(ROOT, f), files)))
            old_asm = dict(zip(present, ex.map(lambda f: compile_asm(old, f), present)))
    print(f"# device assembly, working tree against {sha}: {' '.join(FLAGS[:3])} ... -S --cuda-device-only")
    print("# per kernel: instructions and sha256[:16] of body + .amdhsa_kernel descriptor, <rev> | working tree")
    for f in files:
        if f not in old_asm:
            print(f"\n{f}: not in {sha}  DIFFERENT")
            ndiff += 1
            continue
        lo, ln = normalise(old_asm[f]), normalise(new_asm[f])
        if dump:
            for side, lines in (("old", lo), ("new", ln)):
                with open(os.path.join(dump, f"{f}.{side}.s"), "w") as fh:
                    fh.write("\n".join(lines) + "\n")
        ko, ro = split_kernels(lo)
        kn, rn = split_kernels(ln)
        names = list(ko) + [n for n in kn if n not in ko]
        dm = demangled(names)
        print(f"\n{f}: {len(names)} kernels")
        for n in names:
            o, w = ko.get(n), kn.get(n)
            same = o == w
            ndiff += not same
            nkern += 1
            fmt = lambda x: f"{x[0]:6d} {x[1]}" if x else "     - (absent)        "
            print(f"  {fmt(o)} | {fmt(w)}  {'same' if same else 'DIFFERENT'}  {dm[n]}")
        same = ro == rn
        ndiff += not same
        print(f"  outside the kernels: {ro} | {rn}  {'same' if same else 'DIFFERENT'}")
    print(f"\n{nkern} kernels in {len(files)} files: {ndiff} differences")
    return 1 if ndiff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
