"""What the kernel emulations share: a kernel's own source is compiled for the host against the stand-in runtime of tests/emu
(tests/emu/hip/hip_runtime.h: threads as lanes, real barriers, the MFMAs computed from the lane maps the sources state) together
with its driver tests/emu/<name>_emu.cpp (tests/emu/emu_driver.h: files in and out, buffers between guards), and run as a
stand-alone program, plain or built with AddressSanitizer."""
import shutil
import subprocess
from pathlib import Path

from quantizedsae_amd import build

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "quantizedsae_amd" / "csrc"
EMU = ROOT / "tests" / "emu"
FLAGS = ("-O1", "-std=c++17", "-ffp-contract=off", "-x", "c++", "-pthread")
ASAN_FLAGS = ("-fsanitize=address", "-fno-omit-frame-pointer")


def clangxx() -> str:
    near = Path(build._hipcc()).resolve().parent.parent / "lib" / "llvm" / "bin" / "clang++"
    exe = str(near) if near.exists() else shutil.which("clang++")
    if not exe:
        raise RuntimeError("clang++ (the compiler hipcc drives) not found")
    return exe


def rewrite(text: str, old: str, new: str) -> str:
    assert text.count(old) == 1, old
    return text.replace(old, new)


def compile_emu(build_dir: Path, driver: str, exe_name: str, *, include=(), defines=(), asan=False) -> Path:
    """tests/emu/<driver> -> build_dir/<exe_name>; `include`: where the kernel source is found (csrc, or the directory a test
    wrote its rewritten copy to)."""
    exe = Path(build_dir) / exe_name
    cmd = [clangxx(), *FLAGS, *(ASAN_FLAGS if asan else ()), *(f"-D{d}" for d in defines), f"-I{EMU}",
           *(f"-I{i}" for i in include), str(EMU / driver), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_emu(exe, args, cwd, timeout=900):
    r = subprocess.run([str(exe)] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    return r
