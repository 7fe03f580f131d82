"""No GPU: the host planning and guard code under UndefinedBehaviorSanitizer.  tools/host_guards_ubsan.hip is a stand-alone
program (its own main) that calls the host-only queries over the sweep of tests/test_addressing_cpu.py and with dimensions
up to INT_MAX / 2; it is built here from csrc/*.hip with the sanitizer on the host side only
(`-Xarch_host -fsanitize=undefined -Xarch_host -fno-sanitize-recover=undefined`) into a temporary directory and run on the
CPU.  Nothing of it is loaded into Python.  The first run found `int nrows = N * H` in yolo_dw_wgrad_nslab and the `int`
products k * k * C of the conv plan queries; both are fixed in csrc/."""
import glob
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "custom-yolo-implmentation_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-Xarch_host", "-fsanitize=undefined", "-Xarch_host",
         "-fno-sanitize-recover=undefined", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-DYOLO_ABI_HASH=1L"]


def test_host_guards_have_no_undefined_behaviour(tmp_path):
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.hip"))) + [os.path.join(ROOT, "tools", "host_guards_ubsan.hip")]

    def compile_one(src):
        obj = str(tmp_path / (os.path.basename(src)[:-4] + ".o"))
        r = subprocess.run([HIPCC] + FLAGS + ["-c", src, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, f"hipcc failed on {src}:\n{r.stderr[-3000:]}"
        return obj

    with ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0)))) as ex:
        objs = list(ex.map(compile_one, srcs))
    prog = str(tmp_path / "host_guards_ubsan")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-fsanitize=undefined"] + objs + ["-o", prog], capture_output=True, text=True)
    assert r.returncode == 0, "link failed:\n" + r.stderr[-3000:]
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr, f"status {r.returncode}\n{r.stdout[-1000:]}\n{r.stderr[-3000:]}"
    assert "no undefined behaviour reported" in r.stdout
