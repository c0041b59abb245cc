"""Device code of one .hip file at two revisions, compared symbol by symbol.

    python tools/device_asm_diff.py csrc/kernels/gemm.hip HEAD WORKTREE

Each revision's csrc/kernels is exported to a scratch directory (WORKTREE: the
files as they are on disk), the file is compiled with the kernel flags of
ops/build.py plus `--cuda-device-only -S`, and the assembly is cut where each
function begins (code, kernel descriptor and resource comments stay together),
at every object and at every kernel entry of the `amdgpu_metadata` note.  Emission order may differ between the two, so local
labels lose their function number before chunks are compared by symbol.  The
exit status is 0 when the two symbol sets and every chunk are equal; differing
symbols are listed with a unified diff of their first differing chunk.
"""
from __future__ import annotations

import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")
# ops/build.py kflags
KFLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-munsafe-fp-atomics", "-Wno-unused-result"]

BEGIN = re.compile(r"; -- Begin function (\S+)")
TYPE = re.compile(r"^\s*\.type\s+([^,\s]+),@(?:function|object)")
# local labels carry the function's emission number, the compilation-unit id a hash of the source file
# (label names, loop comments and, through the label's length, the comment column follow from those)
LOCAL = re.compile(r"(\.L(?:BB|func_begin|func_end|tmp)|\bBB(?=\d+_\d)|__hip_cuid_)[0-9a-f]+")
COMMENT_COLUMN = re.compile(r"\s+;")
META = re.compile(r"^  - \.")
NAME = re.compile(r"^    \.name:\s+(\S+)")


def assemble(path: str, rev: str, tmp: str) -> str:
    """Assembly text of `path` (relative to the repository) at `rev`."""
    src_dir = os.path.dirname(path)
    out = os.path.join(tmp, re.sub(r"\W", "_", rev))
    os.makedirs(out)
    if rev == "WORKTREE":
        shutil.copytree(os.path.join(ROOT, src_dir), os.path.join(out, src_dir))
    else:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, src_dir], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", out], input=tar, check=True)
    asm = os.path.join(out, "device.s")
    subprocess.run([HIPCC] + KFLAGS + ["--cuda-device-only", "-S", os.path.join(out, path), "-o", asm], check=True)
    with open(asm) as f:
        return f.read()


def chunks(asm: str) -> dict:
    """{symbol: [lines]}: code and kernel descriptor per symbol, `meta:<kernel>` per metadata entry."""
    raw, key, in_meta = {}, "<header>", False
    for line in asm.splitlines():
        line = COMMENT_COLUMN.sub(" ;", LOCAL.sub(lambda x: x.group(1), line))
        if line.strip() == ".amdgpu_metadata":
            in_meta, key = True, "<metadata>"
        elif line.strip() == ".end_amdgpu_metadata":
            in_meta, key = False, "<trailer>"
        elif in_meta and (META.match(line) or not line.startswith(" ")):
            key = len(raw)  # named below by the entry's .name
        elif not in_meta and ".AMDGPU.gpr_maximums" in line:
            key = "<gpr maximums>"  # once per file, after whichever function came last
        elif not in_meta and (BEGIN.search(line) or TYPE.match(line)):
            prev, key = raw.get(key, []), (BEGIN.search(line) or TYPE.match(line)).group(1)
            if key not in raw and prev and prev[-1].lstrip().startswith(".section"):
                raw[key] = [prev.pop()]  # the function's own section directive precedes its first mention
        raw.setdefault(key, []).append(line)
    out = {}
    for k, lines in raw.items():
        names = [NAME.match(l).group(1) for l in lines if NAME.match(l)]
        out[k if isinstance(k, str) else "meta:" + (names[0] if names else lines[0])] = lines
    assert len(out) == len(raw), "two chunks under one name"
    return out


def main(argv) -> int:
    if len(argv) != 4:
        print(__doc__)
        return 2
    path, rev_a, rev_b = argv[1:]
    with tempfile.TemporaryDirectory() as tmp:
        a, b = (chunks(assemble(path, r, tmp)) for r in (rev_a, rev_b))
    kernels = [k for k in a if k.startswith("meta:_Z")]
    print(f"{path}: {rev_a} {len(a)} symbols ({len(kernels)} kernels), {rev_b} {len(b)} symbols")
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    for name, only in ((rev_a, only_a), (rev_b, only_b)):
        for s in only:
            print(f"only in {name}: {s}")
    differ = [s for s in a if s in b and a[s] != b[s]]
    for s in differ:
        print(f"differs: {s}")
    if differ:
        s = differ[0]
        print("\n".join(list(difflib.unified_diff(a[s], b[s], rev_a, rev_b, lineterm=""))[:80]))
    same = not (only_a or only_b or differ)
    print(f"order of symbols {'equal' if list(a) == list(b) else 'differs'}")
    print("IDENTICAL: every symbol and every chunk equal" if same else "DIFFERENT")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
