"""Machine code of every kernel of the library, one line per kernel, for comparing two trees with `diff`:

    name  size  sha256(disassembly; addresses and the "<symbol+offset>" notes of branch targets stripped)[:16]  vgpr  sgpr  lds  scratch  unit

usage: python tools/kernel_table.py [--debug] [unit.hip ...] > table.txt      (default: every unit of build.SOURCES)

Each unit is compiled device-only with the flags of build.py (--debug: plus -DQSAE_DEBUG_BUILD=1); nothing is written into the
tree.  A kernel's instructions are bounded by its symbol's st_size, so the padding after the last kernel of an ELF is not
counted.  A branch's offset stays in the hash through its encoding; its target note is dropped because it repeats the kernel's
own name, so renaming a kernel changes the first column only.  (Hashes of tables made before that note was dropped do not compare
with these.)  Moving a kernel to another unit must change the last column only; a name listed twice is a kernel emitted twice."""
import hashlib
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from quantizedsae_amd.build import CSRC, FLAGS, SOURCES, _hipcc  # noqa: E402

LLVM = Path(_hipcc()).resolve().parent.parent / "llvm" / "bin"
if not LLVM.exists():
    LLVM = Path("/opt/rocm/llvm/bin")


def _run(*cmd):
    return subprocess.run([str(c) for c in cmd], capture_output=True, text=True, check=True).stdout


def unit_rows(src: str, debug: bool, tmp: str):
    elf = Path(tmp) / (Path(src).stem + ".elf")
    r = subprocess.run([_hipcc()] + FLAGS + (["-DQSAE_DEBUG_BUILD=1"] if debug else []) +
                       ["--cuda-device-only", "--no-gpu-bundle-output", "-c", str(CSRC / src), "-o", str(elf)],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"hipcc failed for {src}:\n{r.stderr}")
    # kernels: the FUNC symbols that have a kernel descriptor (<name>.kd)
    syms, kds = {}, set()
    for line in _run(LLVM / "llvm-readelf", "-sW", "--dyn-syms", elf).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            syms[f[7]] = (int(f[1], 16), int(f[2]))
        elif len(f) == 8 and f[3] == "OBJECT" and f[7].endswith(".kd"):
            kds.add(f[7][:-3])
    kernels = sorted((v[0], v[0] + v[1], n) for n, v in syms.items() if n in kds)
    # instruction stream per kernel: text + encoding of the lines whose address lies inside the symbol
    text = {n: [] for _, _, n in kernels}
    ki = 0
    for line in _run(LLVM / "llvm-objdump", "-d", elf).splitlines():
        m = re.match(r"\s+(.*?)\s*// ([0-9A-F]{12}): (.*)$", line)
        if not m:
            continue
        addr = int(m.group(2), 16)
        while ki < len(kernels) and addr >= kernels[ki][1]:
            ki += 1
        if ki < len(kernels) and addr >= kernels[ki][0]:
            # (a branch's "<symbol+offset>" target note is dropped: it would put the kernel's own name into its hash)
            text[kernels[ki][2]].append(m.group(1) + " | " + re.sub(r"\s*<.*>$", "", m.group(3)))
    # resource fields from the code object's metadata note
    meta = {}
    for block in re.split(r"\n  - (?=\.agpr_count)", _run(LLVM / "llvm-readelf", "--notes", elf)):
        name = re.search(r"^\s+\.name:\s+(\S+)", block, re.M)
        if name:
            meta[name.group(1)] = [re.search(rf"^\s+\.{k}:\s+(\d+)", block, re.M).group(1) for k in
                                   ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")]
    names = _run("c++filt", *[n for _, _, n in kernels]).splitlines()
    return [(dn.replace(" ", ""), hi - lo, hashlib.sha256("\n".join(text[n]).encode()).hexdigest()[:16], *meta[n], src)
            for (lo, hi, n), dn in zip(kernels, names)]


if __name__ == "__main__":
    args = sys.argv[1:]
    debug = "--debug" in args
    units = [a for a in args if a != "--debug"] or SOURCES
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=4) as ex:
        rows = [r for rs in ex.map(lambda u: unit_rows(u, debug, tmp), units) for r in rs]
    for r in sorted(rows):
        print("  ".join(str(c) for c in r))
