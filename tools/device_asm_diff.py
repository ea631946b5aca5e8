"""Compare the gfx950 device assembly of csrc/*.hip in the working tree with that of a git revision.

    python tools/device_asm_diff.py REV [--jobs N]

Each file is compiled on both sides with build._flags(src) plus --cuda-device-only -S (REV's csrc/ comes from
`git archive`).  Lines with the per-compile __hip_cuid_ symbol are dropped and the function numbers in local labels
(.LBB12_3, .Lfunc_end12) are removed, so that a deleted kernel does not renumber its neighbours.  The text is then
compared symbol by symbol (a function's body, its kernel descriptor, its metadata entry): "identical" per file, or the
symbols that differ or exist on one side only.  Exit status 0 only if no symbol of the working tree differs.
"""
import argparse
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "to-ued_amd"))
import build as B  # noqa: E402

START = re.compile(r"^\t\.type\t(\S+),@function|^\t\.amdhsa_kernel (\S+)|^(  - \.)")   # function, descriptor, metadata
LEAD = re.compile(r"^\t\.(section|text|globl|weak|protected|p2align)\b")   # lines in front of a symbol: they go with it
TAIL = re.compile(r"^\t\.section\t\.AMDGPU\.gpr_maximums|^\t\.amdgpu_metadata|^amdhsa\.target")   # file scope again
META_NAME = re.compile(r"^    \.name:\s+(\S+)")
LABEL_NO = re.compile(r"(\.L[A-Za-z_]*[A-Za-z])\d+")


def compile_asm(src: Path, out: Path) -> str:
    flags = [f.replace(str(B.CSRC), str(src.parent)) for f in B._flags(src)]
    cmd = [B.hipcc(), *flags, "--cuda-device-only", "-S", str(src), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{r.stderr}")
    return out.read_text()


def by_symbol(asm: str) -> dict:
    """symbol -> its lines; "" holds the text at file scope."""
    out, key, held, meta = {"": []}, "", [], False   # held: lines whose symbol is not known yet
    for line in asm.splitlines():
        if "__hip_cuid_" in line:
            continue
        line = LABEL_NO.sub(r"\1", line)
        m = START.match(line)
        if TAIL.match(line) or (m and m.group(3)):
            out[key] += held
            key, held, meta = key if m else "", [], bool(m)
        name = META_NAME.match(line) if meta else m
        if name:
            key, meta = name.group(1) or name.group(2), False
        if meta or LEAD.match(line):
            held.append(line)
        else:
            out[key] = out.get(key, []) + held + [line]
            held = []
    out[key] += held
    return out


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    r = subprocess.run([filt, *names], capture_output=True, text=True) if filt and names else None
    return dict(zip(names, r.stdout.splitlines() if r and r.returncode == 0 else names))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("rev")
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        rel = B.CSRC.relative_to(REPO).as_posix()
        tar = subprocess.run(["git", "-C", str(REPO), "archive", a.rev, rel], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", td], input=tar, check=True)
        sides = {"tree": B.CSRC, "rev": Path(td) / rel}
        names = sorted({p.name for d in sides.values() for p in d.glob("*.hip")})
        jobs = [(n, s) for n in names for s in sides if (sides[s] / n).exists()]
        with ThreadPoolExecutor(max_workers=max(1, min(a.jobs, 16))) as ex:
            asm = dict(zip(jobs, ex.map(lambda j: compile_asm(sides[j[1]] / j[0], Path(td) / f"{j[1]}_{j[0]}.s"), jobs)))
    ok = True
    for n in names:
        new, old = (by_symbol(asm[n, s]) if (n, s) in asm else {} for s in ("tree", "rev"))
        diff = sorted(k for k in new.keys() | old.keys() if new.get(k) != old.get(k))
        nice = demangle([k for k in diff if k])
        for k in diff:
            what = "differs" if k in new and k in old else f"only in {'the working tree' if k in new else a.rev}"
            ok &= k not in new
            print(f"{n}: {nice.get(k, '<file scope>')}: {what}")
        if not diff:
            print(f"{n}: identical")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
