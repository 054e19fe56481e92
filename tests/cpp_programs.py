"""What the tests of the C++ side share: the g++ command lines of the stand-alone case programs (plain, and under
AddressSanitizer + UndefinedBehaviorSanitizer) and of the mirror programs that link libspm_hip.so, the C99 programs that
print the header's layouts, and the download of a device view.  A plain module, imported by the test files that need it."""
import ctypes
import os
import pathlib
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIB = os.path.join(ROOT, "libspm_amd")
WARN = ["-Wall", "-Wextra", "-Werror"]
SANITIZE = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def build_cases(source, out_dir, std="c++20", include=(), sanitize=False, threads=False):
    """A host-only case program (its own main, no device, nothing to link): tests/cpp/<source> -> out_dir/<name>, or
    <name>_asan with the sanitizers.  include: directories for -I.  threads: the program starts std::threads."""
    name = os.path.splitext(os.path.basename(source))[0]
    exe = pathlib.Path(out_dir) / (name + ("_asan" if sanitize else ""))
    flags = ["-std=" + std] + (SANITIZE if sanitize else ["-O2", "-pedantic"])
    subprocess.check_call(["g++"] + flags + WARN + (["-pthread"] if threads else []) + ["-I" + d for d in include] +
                          ["-o", str(exe), os.path.join(CPP, source)])
    return exe


def build_mirror(source, out_dir, fixtures=True):
    """A program over the C++ mirror (include/) and libspm_hip.so, with the reference's warning flags: source (a file of
    tests/cpp, or a path) -> out_dir/<name>.  fixtures: it reads the VCF fixtures of tests/golden/jst (SPM_TEST_DATA, zlib)."""
    exe = pathlib.Path(out_dir) / os.path.splitext(os.path.basename(source))[0]
    data = ['-DSPM_TEST_DATA="' + os.path.join(ROOT, "tests", "golden", "jst") + '"'] if fixtures else []
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-pedantic"] + WARN + ["-I" + os.path.join(ROOT, "include")] + data +
                          ["-o", str(exe), os.path.join(CPP, source), "-L" + LIB, "-l:libspm_hip.so", "-Wl,-rpath," + LIB,
                           "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"] + (["-lz"] if fixtures else []))
    return exe


def c_layout(tmp_path, source):
    """What a C99 program over include/spm_hip.h (its own main, nothing to link) prints about the header's layouts:
    source -> tmp_path/layout, run; its lines "<name> <value>" -> {name: value}, the values as printed."""
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(source)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic"] + WARN + ["-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    return dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())


def download(ctx, device_ptr, n, dtype):
    """n records of dtype at device_ptr, behind everything the context has enqueued"""
    dtype = np.dtype(dtype)
    out = np.zeros(n, dtype=dtype)
    if n:
        ctx.synchronize()
        hip = ctypes.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(device_ptr), dtype.itemsize * n, 2) == 0
    return out
